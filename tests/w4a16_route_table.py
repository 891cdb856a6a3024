"""The w4a16 GEMM route table shared by tests/test_gpu_w4a16_routes.py (the kernels against the oracle, with the
route each shape takes asserted) and tests/test_cpu_w4a16_route_shapes.py (the oracle against an independent
high-precision value at the same shapes), so that the two cannot drift.

run_gemm_t (vllm_metax_amd/csrc/w4a16.hip) sends a 4-bit GEMM to one of:
  n % 64 != 0                                              -> any-N kernel                      ANY_N4
  m >= 1024 with scratch for both operand images           -> operand-image GEMM                IMAGE | PACK_A
  stripe shape (k % 128 == 0, group 32 / 64 / 128 j)       -> stripe kernel, passes <= 128 rows STRIPE
  m >= 128, not a stripe shape, k % 64 == 0                -> 128 x 256 tile kernel             LARGE_M
  everything else                                          -> small-M kernel, <= 64 rows a call SMALL_M
plus PACK_A when the activations were re-tiled first and SUM_SLABS when K was split across workgroups.

A row is (quant, bits, m, k, n, group, with_temp_space, expected_route_bits); quant is one of
  awq        awq_gemm through _custom_ops
  gptq       gptq_gemm, asymmetric zeros;  gptq_sym: stored zero 7;  gptq_act: act-order (g_idx + perm_space)
  awq_raw    mi355x_awq_gemm through the C-ABI with NO dequant scratch (the small-M kernel without PACK_A)
  awq_tight  the same with a scratch of exactly roundup(m, 16) * k * 2 bytes: enough for the image of a 1- or
             2-tile call; a 3-tile call (33..48 rows) runs the 4-tile kernel, whose image does not fit
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.util import ROOT  # noqa: F401  (puts the repository root on sys.path)
from oracle import ref_ops as R  # noqa: E402

# MI355X_W4_ROUTE_* of include/mi355x_hotpath.h (test_cpu_w4a16_route_shapes.py compares them with the header)
STRIPE, SMALL_M, LARGE_M, IMAGE, ANY_N4, ANY_8, PACK_A, SUM_SLABS = 1, 2, 4, 8, 16, 32, 64, 128
ROUTE_BITS = {"STRIPE": STRIPE, "SMALL_M": SMALL_M, "LARGE_M": LARGE_M, "IMAGE": IMAGE, "ANY_N4": ANY_N4,
              "ANY_8": ANY_8, "PACK_A": PACK_A, "SUM_SLABS": SUM_SLABS}
# kernels no later change of the router may leave without a row
MUST_COVER = SMALL_M | LARGE_M | ANY_N4 | PACK_A | SUM_SLABS | STRIPE


def route_names(mask: int) -> str:
    return "|".join(name for name, bit in ROUTE_BITS.items() if mask & bit) or "0"


def _rows():
    rows = []

    def add(quant, m, k, n, group, ts, route):
        assert k % 32 == 0 and n % 8 == 0 and group % 32 == 0 and k % group == 0
        rows.append((quant, 4, m, k, n, group, ts, route))

    # ---- any-N kernel (n % 64 != 0): 16 columns x 8 rows per workgroup, 16 k-parts striding k / 8 words.
    # n not a multiple of 16 (8, 24, 72, 200); k = 1056: 132 words, 8 or 9 iterations per k-part; m at the edges
    # of the 8-row blocks; groups 32, 96 (not a power of two) and k; both zero-point modes.
    i = 0
    for quant in ("awq", "gptq"):
        for n in (8, 24, 72, 200):
            for k, group in ((32, 32), (160, 32), (160, 160), (1056, 32), (1056, 1056), (96, 96), (288, 96)):
                add(quant, (1, 8, 9, 70)[i % 4], k, n, group, False, ANY_N4)
                i += 1
    add("awq", 1030, 64, 72, 32, False, ANY_N4)        # n % 64 != 0 wins over the m >= 1024 branch
    add("gptq_act", 9, 160, 72, 32, False, ANY_N4)

    # ---- small-M kernel, m <= 64 (the stripe kernel declines: k % 128 != 0, or group 96): MT = 1, 2, 4 and the
    # 3-tile case that runs as MT = 4; groups that are no power of two; its own split-K (k = 1056 / 2080: 33 / 65
    # k-steps in 2 / 4 uneven splits) only with a temp_space.
    combos = ((32, 32, False), (96, 32, False), (96, 96, False), (160, 32, False), (160, 160, False),
              (160, 32, True), (288, 96, False), (384, 96, False), (1056, 32, False), (1056, 32, True),
              (2080, 32, False), (2080, 32, True))
    for c, (k, group, ts) in enumerate(combos):
        for j, m in enumerate((1, 16, 17, 33, 49, 64)):
            route = SMALL_M | PACK_A | (SUM_SLABS if ts and k >= 1024 else 0)
            add(("awq", "gptq_sym", "gptq")[(c + 2 * j) % 3], m, k, (64, 192, 320)[(c + j) % 3], group, ts, route)
    add("awq_raw", 1, 96, 64, 96, False, SMALL_M)
    add("awq_raw", 33, 160, 192, 32, False, SMALL_M)
    add("awq_raw", 64, 1056, 64, 32, True, SMALL_M | SUM_SLABS)
    add("awq_raw", 100, 1056, 64, 32, False, SMALL_M)              # two halves, no scratch to alias: no split
    add("awq_tight", 17, 160, 64, 32, False, SMALL_M | PACK_A)
    add("awq_tight", 33, 160, 64, 32, False, SMALL_M)

    # ---- 65..127 rows, stripe declined: two halves of <= 64 rows on the small-M kernel.  Without a temp_space the
    # split-K slabs live in the dequant scratch, which also holds the packed activations: the k >= 1024 rows
    # without temp_space are the ones where the two must not overlap.
    i = 0
    for m in (65, 100, 127):
        for k in (160, 1056, 2080):
            for n in (64, 256):
                for ts in (False, True):
                    add(("awq", "gptq", "gptq_sym")[i % 3], m, k, n, 32, ts,
                        SMALL_M | PACK_A | (SUM_SLABS if k >= 1024 else 0))
                    i += 1

    # ---- 128 x 256 tile kernel (128 <= m < 1024, not a stripe shape, k % 64 == 0): ragged M, inactive column
    # waves (n = 64, 320, 576) and partial 256-column tiles, one k tile (k = 64), a group of 32 inside the 64-k tile.
    i = 0
    for k, group in ((64, 32), (64, 64), (192, 32), (192, 64), (192, 192), (1088, 32), (1088, 64), (1088, 1088),
                     (384, 96)):
        for j, m in enumerate((128, 129, 300, 1000)):
            add(("awq", "gptq", "gptq_sym")[i % 3], m, k, (64, 256, 320, 576)[(i // 4 + j) % 4], group,
                i % 2 == 1, LARGE_M)
            i += 1

    # ---- m >= 128 and k % 64 != 0: the tile kernel declines too, 64-row halves on the small-M kernel
    for quant in ("awq", "gptq"):
        for m in (128, 200):
            add(quant, m, 96, 256, 32 if quant == "awq" else 96, False, SMALL_M | PACK_A)
            add(quant, m, 1056, 256, 32, False, SMALL_M | PACK_A | SUM_SLABS)
    add("awq", 150, 1056, 256, 32, False, SMALL_M | PACK_A | SUM_SLABS)   # last pass of 22 rows: no halves

    # ---- GPTQ on the stripe kernel: groups other than 128 (4, 2 and 1 scale sets per 128-k stage), 65..128-row
    # passes.  The planner splits K of the narrow k = 1024 shape and not of k = 512 (plan_stripe's cost model).
    i = 0
    for group in (32, 64, 256):
        for m in (100, 128, 300):
            for k, n in ((512, 256), (1024, 192)):
                add(("gptq", "gptq_sym")[i % 2], m, k, n, group, i % 4 == 3, STRIPE | (SUM_SLABS if k >= 1024 else 0))
                i += 1
    add("gptq_act", 100, 512, 256, 64, False, STRIPE)
    return rows


ROWS = _rows()
assert len(set(r[:-1] for r in ROWS)) == len(ROWS), "route table: a shape is listed twice"
DTYPES = (torch.bfloat16, torch.float16)


def row_id(row) -> str:
    quant, _, m, k, n, group, ts, _ = row
    return f"{quant}-m{m}-k{k}-n{n}-g{group}-{'ws' if ts else 'nows'}"


def make_awq(k, n, group, dtype, seed=0):
    """As tests/test_gpu_w4a16.py: nibbles and zeros U{0..15}, scales U(1e-3, 1e-2)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 16, size=(k, n), dtype=np.uint8)
    z = rng.integers(0, 16, size=(k // group, n), dtype=np.uint8)
    g = torch.Generator().manual_seed(seed)
    scales = (torch.rand(k // group, n, generator=g) * 9e-3 + 1e-3).to(dtype)
    return R.awq_pack(w), R.awq_pack(z), scales, w, z


def make_gptq(k, n, group, dtype, seed=0, sym=False):
    """As tests/test_gpu_w4a16.py (stored zeros U{0..14} or the symmetric 7; the kernels add 1), plus the raw integers."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 16, size=(k, n), dtype=np.uint8)
    z = np.full((k // group, n), 7, dtype=np.uint8) if sym else \
        rng.integers(0, 15, size=(k // group, n), dtype=np.uint8)
    g = torch.Generator().manual_seed(seed)
    scales = (torch.rand(k // group, n, generator=g) * 9e-3 + 1e-3).to(dtype)
    qz = torch.from_numpy(R._pack_nibbles(z.reshape(k // group, n // 8, 8)).view(np.int32))
    return R.gptq_pack_rows(w), qz, scales, w, z


@functools.lru_cache(maxsize=None)
def case(index: int, dtype):
    """Inputs of ROWS[index] in `dtype` and the oracle's result, computed once; callers must not modify them."""
    quant, bits, m, k, n, group, _, _ = ROWS[index]
    assert bits == 4
    seed = 1000 + index
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(seed + 1)) * 0.5).to(dtype)
    c = SimpleNamespace(x=x, perm=None)
    if quant.startswith("awq"):
        c.qw, c.qz, c.sc, c.w, c.z = make_awq(k, n, group, dtype, seed=seed)
        c.ref = R.awq_gemm(x, R.awq_to_gptq_4bit(c.qw), c.sc, c.qz)
    else:
        c.qw, c.qz, c.sc, c.w, c.z = make_gptq(k, n, group, dtype, seed=seed, sym=quant == "gptq_sym")
        if quant == "gptq_act":
            c.perm = torch.randperm(k, generator=torch.Generator().manual_seed(seed + 2)).to(torch.int32)
        c.ref = R.gptq_gemm(x, R.gptq_shuffle(c.qw, c.perm), c.qz, c.sc, c.perm, group)
    return c
