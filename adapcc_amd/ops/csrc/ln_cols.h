// The row widths the row-per-wave kernels are instantiated for (LayerNorm in
// lnorm.hip, the GeLU backward with column sums in gelu.hip): the width is a
// template parameter there, so a lane's slice of a row, and what it sums down
// its columns, sits in registers under static indexing.
#pragma once

#define LN_COLS_LIST(X) \
  X(128) X(256) X(384) X(512) X(640) X(768) X(1024) X(1280) X(1536) \
  X(2048) X(3072) X(4096)
