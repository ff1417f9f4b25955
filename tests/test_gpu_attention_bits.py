"""Output bits of the flash-attention kernels (csrc/attn.hip), pinned.

Every output of a fixed set of cases is hashed (sha256 of the raw bytes) and
compared with tests/golden/attn_bits.json. That file was recorded on an
MI355X from commit 2ffa911, the last one before the kernels' staging,
epilogue and launch code was folded into shared helpers; it is never
regenerated from later code, so a change to the tile loop that moves a
single bit of o, lse, delta or a gradient fails here. Inputs come from a
fixed integer LCG, not from an RNG, so the fixture does not depend on the
torch version.

The cases cover all nine kernel instantiations: causal, non-causal with
S % 128 == 0, and ragged lengths with a skipped half-tile (S = 1, 65), a
second workgroup that holds a single row (129) and a prefetch with one
valid row (65, 129, 197); the packed cases add the strided layouts.

``python tests/test_gpu_attention_bits.py --record`` rewrites the json. Only
do that on purpose, for a change that is meant to alter the arithmetic.
"""

import hashlib
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 64
SCALE = 1.0 / math.sqrt(D)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attn_bits.json")

# name -> (causal, B, H, S), through _launch_fwd / _launch_bwd
UNPACKED = {
    "causal_1x2x128": (True, 1, 2, 128),
    "causal_2x3x256": (True, 2, 3, 256),
    "noncausal_1x2x128": (False, 1, 2, 128),
    "ragged_2x3x1": (False, 2, 3, 1),
    "ragged_2x3x65": (False, 2, 3, 65),
    "ragged_2x3x129": (False, 2, 3, 129),
    "ragged_2x3x197": (False, 2, 3, 197),
}
# name -> (causal, B, n_head, T), through flash_attention_qkv
PACKED = {
    "packed_causal_2x3x256": (True, 2, 3, 256),
    "packed_noncausal_2x3x197": (False, 2, 3, 197),
}

# LCG (multiplier, increment) per tensor
LCG = {"q": (1103515245, 12345), "k": (1664525, 1013904223),
       "v": (22695477, 1), "do": (134775813, 1013), "qkv": (214013, 2531011)}


def lcg_bf16(shape, which):
    """4001 levels in [-2, 2] (1269 distinct once rounded to bf16), built
    on the CPU with integer arithmetic only, then copied to the device."""
    a, c = LCG[which]
    n = math.prod(shape)
    x = (torch.arange(n, dtype=torch.int64) * a + c) % (1 << 31)
    x = (x >> 8) % 4001
    return ((x - 2000).double() / 1000.0).to(torch.bfloat16).view(shape).cuda()


def digest(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def run_unpacked(causal, B, H, S):
    from adapcc_amd.ops.attention import _launch_bwd, _launch_fwd

    shape = (B, H, S, D)
    q, k, v, do = (lcg_bf16(shape, n) for n in ("q", "k", "v", "do"))
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    lse = torch.empty((B, H, S), dtype=torch.float32, device="cuda")
    delta = torch.empty_like(lse)
    _launch_fwd(q, k, v, o, lse, SCALE, causal=causal)
    _launch_bwd(q, k, v, o, do, lse, dq, dk, dv, SCALE, causal=causal,
                delta=delta)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "delta": delta, "dq": dq, "dk": dk, "dv": dv}


def run_packed(causal, B, n_head, T):
    from adapcc_amd.ops.attention import fa_qkv_supported, flash_attention_qkv

    C = n_head * D
    qkv = lcg_bf16((B, T, 3 * C), "qkv").requires_grad_(True)
    dy = lcg_bf16((B, T, C), "do")
    assert fa_qkv_supported(qkv, n_head, 0.0, causal=causal)
    y = flash_attention_qkv(qkv, n_head, causal=causal)
    y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y, "dqkv": qkv.grad}


def run_case(name):
    outs = (run_unpacked(*UNPACKED[name]) if name in UNPACKED
            else run_packed(*PACKED[name]))
    return {tensor: digest(t) for tensor, t in outs.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", list(UNPACKED) + list(PACKED))
def test_output_bits(name, golden):
    got = run_case(name)
    want = golden[name]
    assert sorted(got) == sorted(want), f"{name}: tensor set changed"
    for tensor in got:
        assert got[tensor] == want[tensor], (
            f"{name}: {tensor} differs from the recorded bits")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_attention_bits.py --record")
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    cases = {name: run_case(name) for name in list(UNPACKED) + list(PACKED)}
    with open(GOLDEN, "w") as f:
        json.dump({"recorded_from": "2ffa911", "cases": cases}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print("recorded", len(cases), "cases to", GOLDEN)
