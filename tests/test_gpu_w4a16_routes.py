"""GPU parity of EVERY route of the 4-bit w4a16 GEMM (run_gemm_t, vllm_metax_amd/csrc/w4a16.hip) against the CPU
oracle, with the route asserted: each row of tests/w4a16_route_table.py names the kernels its call must launch
(mi355x_w4a16_last_route), so a change of the router that stops sending shapes to a kernel fails here instead of
silently leaving that kernel untested.

Bounds: tests.util.assert_gemm_close at its defaults (1 ulp of the output type + 2e-4 max|ref|, at most 5 % of the
elements different); the oracle's own error at these shapes is pinned by tests/test_cpu_w4a16_route_shapes.py.
Scratch contents must not matter: temp_space is filled with NaN and the op surface's dequant scratch with 0xFF
bytes (NaN as bf16 / f16 / f32) before every call.
"""
import pytest
import torch

from tests.util import assert_bit_exact, assert_gemm_close, dev
from tests.w4a16_route_table import (DTYPES, MUST_COVER, PACK_A, ROWS, SMALL_M, SUM_SLABS, case, route_names,
                                     row_id)

pytestmark = pytest.mark.gpu

# collection time: the table still reaches every kernel (a row whose route moved has to be replaced, not dropped)
_union = 0
for _row in ROWS:
    _union |= _row[-1]
assert _union & MUST_COVER == MUST_COVER, f"route table: no row for {route_names(MUST_COVER & ~_union)}"


def ops():
    from vllm_metax_amd import _custom_ops
    return _custom_ops


@pytest.fixture(scope="module", autouse=True)
def scratch():
    """The op surface's per-device dequant scratch only ever grows, and what fits into it decides PACK_A and the
    K splits: grow it once to 4 MiB (every shape here needs far less), so that a row's route does not depend on
    the tests that ran before it."""
    return ops()._dq_scratch(64, 64, 1 << 15, dev())


def _raw_awq_gemm(x, q2, sc, qz, ws, dq):
    """mi355x_awq_gemm through the C-ABI, with the dequant scratch the caller chooses (None: null pointer)."""
    from vllm_metax_amd import _abi
    m, k = x.shape
    n = q2.size(0)
    out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    rc = _abi.load().mi355x_awq_gemm(
        out.data_ptr(), x.data_ptr(), q2.data_ptr(), sc.data_ptr(), qz.data_ptr(),
        ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
        dq.data_ptr() if dq is not None else None, dq.numel() if dq is not None else 0,
        m, n, k, k // sc.size(0), x.stride(0), _abi.BF16 if x.dtype == torch.bfloat16 else _abi.F16,
        torch.cuda.current_stream().cuda_stream)
    _abi.check(rc, "awq_gemm")
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("index", range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_route(index, dtype, scratch):
    quant, bits, m, k, n, group, with_ws, route = ROWS[index]
    what = row_id(ROWS[index])
    c = case(index, dtype)
    d = dev()
    bf16 = dtype == torch.bfloat16
    x, qz, sc = c.x.to(d), c.qz.to(d), c.sc.to(d)
    ws = torch.full((8 * m * n,), float("nan"), dtype=torch.float32, device=d) if with_ws else torch.empty(0)
    if quant.startswith("awq"):
        qw = ops().awq_to_gptq_4bit(c.qw.to(d))
        if quant == "awq":
            call = lambda: ops().awq_gemm(x, qw, qz, sc, 8, ws, bf16)   # noqa: E731
        else:
            tight = torch.empty((m + 15) // 16 * 16 * k * 2, dtype=torch.uint8, device=d) \
                if quant == "awq_tight" else None
            call = lambda: _raw_awq_gemm(x, qw, sc, qz, ws if with_ws else None, tight)   # noqa: E731
    else:
        qw = c.qw.to(d).clone()
        perm = c.perm.to(d) if c.perm is not None else torch.empty(0, dtype=torch.int32, device=d)
        ops().gptq_shuffle(qw, perm, bits)
        pspace = torch.empty(m, k, dtype=dtype, device=d) if c.perm is not None else torch.empty(0)
        call = lambda: ops().gptq_gemm(x, qw, qz, sc, perm, True, bits, group, pspace, ws, bf16)   # noqa: E731
    scratch.fill_(0xFF)
    out = call()
    got = ops().w4a16_last_route()
    assert got == route, f"{what}: route {route_names(got)}, expected {route_names(route)}"
    assert_gemm_close(out, c.ref, what)
    if m > 64 and not with_ws and route & SMALL_M and route & SUM_SLABS and route & PACK_A:
        # the split-K slabs and the packed activations share the dequant scratch: they must not overlap (slab
        # stores of one workgroup over activations another has yet to read would show as run-to-run variation)
        for rep in range(2):
            scratch.fill_(0xFF)
            assert_bit_exact(call(), out, f"{what}: repeat {rep + 1}")
