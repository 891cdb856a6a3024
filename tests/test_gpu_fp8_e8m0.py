"""GPU parity: the E8M0-scaled fp8 GEMM behind cutlass_scaled_mm (e4m3 operands, float8_e8m0fnu scales on both sides,
applied inside the scaled MFMA) in its block form ([m, k / 128] x [k / 128, ceil(n / 128)]) and its MX form
([m, k / 32] x [k / 32, n]), and per_token_group_quant_fp8 with scale_ue8m0.

Reference: the contract restated in float64 on the CPU — e4m3 decoded, multiplied by 2^(byte - 127) repeated over the
group or block, ONE matmul, the bias, one rounding.  Tolerance of the random cases: tests.util.assert_gemm_close with
its default `rel` (the per-element bound) and a cap on the fraction of elements that differ at all.  Measured on an
MI355X over the cases of test_e8m0_scaled_mm: f16 differs in at most 6.39 % (block 6.36 %, mx 6.39 %), inside the 9 %
tests/test_gpu_fp8_gemm.py carries for this MFMA's internal adder; bf16 differs in 0.88 - 1.17 % at every shape of
4352 elements or more, but 1 x 16 x 128 has 16 outputs and one rounding flip there (mx, no bias) is 6.25 %, beyond
that file's 3 %: the bf16 cap is that worst fraction x 1.5.  test_scale_placement_is_exact is the guard no cap
loosens.  Every case asserts the kernel the router took (scaled_mm_fp8_e8m0_last_route)."""
import pytest
import torch

from tests.util import assert_bit_exact, assert_gemm_close, dev

pytestmark = pytest.mark.gpu

F8, E8 = torch.float8_e4m3fn, torch.float8_e8m0fnu
STREAM, TILE, SLABS = 1, 2, 4
MAX_FRAC = {torch.float16: 0.09, torch.bfloat16: 0.0625 * 1.5}
T = 65                                     # the router's threshold: m <= T streams (profiles/fp8_e8m0_gemm.txt)


def ops():
    from vllm_metax_amd import _custom_ops
    return _custom_ops


def _scale_shapes(form, m, n, k):
    """(a_s, b_s as the checkpoint stores it: [n, k / 32] or [ceil(n / 128), k / 128])"""
    return ((m, k // 32), (n, k // 32)) if form == "mx" else ((m, k // 128), ((n + 127) // 128, k // 128))


def _ref(form, a, b_nk, a_s, b_s, out_dtype, bias=None):
    group = 32 if form == "mx" else 128
    sb = torch.pow(2.0, b_s.view(torch.uint8).double() - 127).repeat_interleave(group, 1)
    if form == "block":
        sb = sb.repeat_interleave(128, 0)[:b_nk.shape[0]]
    sa = torch.pow(2.0, a_s.view(torch.uint8).double() - 127).repeat_interleave(group, 1)
    r = (a.view(F8).double() * sa) @ (b_nk.view(F8).double() * sb).t()
    return (r + bias.double() if bias is not None else r).to(out_dtype)


def _run(a, b_nk, a_s, b_s, bias, out_dtype, op=None):
    d = dev()
    out = torch.full((a.shape[0], b_nk.shape[0]), float("nan"), dtype=out_dtype, device=d)
    (op or ops().cutlass_scaled_mm)(out, a.to(d).view(F8), b_nk.to(d).view(F8).t(), a_s.to(d).view(E8),
                                    b_s.to(d).view(E8).t(), bias.to(d) if bias is not None else None)
    return out, ops().scaled_mm_fp8_e8m0_last_route()


def _operands(form, m, n, k, g, values=None, spread=(-6, 0)):
    if values is None:
        a, b_nk = ((torch.randn(r, k, generator=g) * 2).clamp(-448, 448).to(F8) for r in (m, n))
    else:
        c = torch.tensor(values).to(F8)
        a, b_nk = (c[torch.randint(len(values), (r, k), generator=g)] for r in (m, n))
    a_s, b_s = ((127 + torch.randint(*spread, shape, generator=g)).to(torch.uint8)
                for shape in _scale_shapes(form, m, n, k))
    return a, b_nk, a_s, b_s


# (m, n, k) -> the route: kernel bit, + SLABS where the plan splits K
SHAPES = {
    (1, 16, 128): STREAM,                     # one k-step: a ragged super-step of r = 1
    (16, 272, 384): STREAM,                   # r = 3, ragged last column block, n no multiple of 128
    (33, 576, 1024): STREAM,                  # ragged rows, two whole super-steps
    (64, 1280, 8192): STREAM | SLABS,         # K split through slabs
    (65, 256, 640): STREAM,                   # a second pass of one row
    (T, 512, 512): STREAM,                    # both sides of the router's threshold
    (T + 1, 512, 512): TILE,
    (333, 320, 1152): TILE | SLABS,           # 9 k-steps over uneven splits
    (1030, 272, 384): TILE,                   # ragged in m and n, odd number of k-steps
}


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("m,n,k", list(SHAPES))
@pytest.mark.parametrize("form", ["block", "mx"])
def test_e8m0_scaled_mm(form, m, n, k, bias, out_dtype):
    g = torch.Generator().manual_seed(0)
    a, b_nk, a_s, b_s = _operands(form, m, n, k, g)
    bi = (torch.rand(n, generator=g) * 2 - 1).to(out_dtype) if bias else None
    out, route = _run(a, b_nk, a_s, b_s, bi, out_dtype)
    assert route == SHAPES[m, n, k], f"{m}x{n}x{k}: route {route}"
    assert_gemm_close(out, _ref(form, a, b_nk, a_s, b_s, out_dtype, bi), f"e8m0 {form} {m}x{n}x{k}",
                      max_frac=MAX_FRAC[out_dtype])


@pytest.mark.parametrize("m,n,k,route", [
    (40, 272, 640, STREAM), (64, 1280, 8192, STREAM | SLABS),
    (8, 272, 2432, STREAM),                   # 5 super-steps in one range: the register ring goes round, r = 3
    (24, 4112, 8192, STREAM | SLABS),         # two column tiles per wave
    (T + 10, 272, 640, TILE), (333, 320, 1152, TILE | SLABS)])
@pytest.mark.parametrize("form", ["block", "mx"])
def test_scale_placement_is_exact(form, m, n, k, route):
    """Operands from {0, +-0.5, +-1, +-2} and scale bytes 127 + {-1, 0, 1}, independent per (row, group) and per
    (column, group) or weight block, integer bias: every product is a multiple of 2^-4 and a partial sum stays below
    2^17 even at K = 8192 — exact in fp32 in any order, so the result must EQUAL the float64 reference.  A scale byte
    taken from the wrong row, column, group, block or op_sel position cannot hide inside a tolerance."""
    g = torch.Generator().manual_seed(m)
    a, b_nk, a_s, b_s = _operands(form, m, n, k, g, values=[0, .5, -.5, 1, -1, 2, -2], spread=(-1, 2))
    bi = torch.randint(-8, 9, (n,), generator=g).to(torch.bfloat16)
    out, got_route = _run(a, b_nk, a_s, b_s, bi, torch.bfloat16)
    assert got_route == route
    assert_bit_exact(out, _ref(form, a, b_nk, a_s, b_s, torch.bfloat16, bi), f"placement {form} m={m}")


def _quant_ref(x, group, eps=1e-10):
    """The rule of the contract, restated: (e4m3 [tokens, hidden], scale bytes [tokens, hidden / group])"""
    tokens, hidden = x.shape
    xg = x.float().view(tokens, hidden // group, group)
    s0 = xg.abs().amax(-1).clamp(min=eps) / 448
    b = s0.view(torch.int32)
    byte = ((b >> 23) + ((b & 0x7FFFFF) != 0)).clamp(max=254)
    return torch.ldexp(xg, (127 - byte)[..., None]).to(F8).view(tokens, hidden), byte.to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("column_major", [False, True])
@pytest.mark.parametrize("scale_dtype", [torch.float32, E8])
@pytest.mark.parametrize("group", [32, 128])
@pytest.mark.parametrize("tokens,hidden", [(7, 512), (300, 4096)])
def test_per_token_group_quant_fp8_ue8m0(tokens, hidden, group, scale_dtype, column_major, dtype):
    g = torch.Generator().manual_seed(hidden)
    x = (torch.randn(tokens, hidden, generator=g) * torch.rand(tokens, 1, generator=g) * 8).to(dtype)
    x[0, :group] = 0                                                # an all-zero group: the eps clamp
    x[1, :group] = x[1, :group].clamp(-1, 1)
    x[1, 3] = 56                                                    # absmax 448 * 2^-3: mantissa 0, no round-up
    x[2, group:2 * group] = x[2, group:2 * group].clamp(-1, 1)      # just above: round-up to 2^-2, then 8.5 and 9.5
    x[2, group:group + 3] = torch.tensor([56.25, 2.125, -2.375]).to(dtype)   # are e4m3 ties (-> 8, -10)
    q, s = ops().per_token_group_quant_fp8(x.to(dev()), group, column_major_scales=column_major, scale_ue8m0=True,
                                           scale_dtype=scale_dtype)
    assert q.dtype == F8 and s.dtype == scale_dtype and s.shape == (tokens, hidden // group)
    assert s.stride(0) == (1 if column_major else hidden // group)
    want_q, want_s = _quant_ref(x, group)
    assert want_s[0, 0] == 85 and want_s[1, 0] == 124 and want_s[2, 1] == 125
    assert want_q[2, group:group + 3].float().tolist() == [224, 8, -10]
    if scale_dtype == E8:
        assert_bit_exact(s.view(torch.uint8), want_s, "group scale bytes")
    else:
        assert_bit_exact(s, torch.ldexp(torch.ones(()), want_s.int() - 127), "group scales")
    assert_bit_exact(q.view(torch.uint8), want_q.view(torch.uint8), "quantised values")


def test_linears_and_torch_ops():
    """quant_config.linear.apply_fp8_block with byte scales and apply_mxfp8 = group quantiser + GEMM on the
    checkpoint's own tensors; against the float64 reference on the quantiser's own bytes.  The torch.ops._C forms give
    the same bits."""
    from vllm_metax_amd.quant_config import linear
    import vllm_metax_amd._C  # noqa: F401
    d = dev()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 20, 512, generator=g).to(torch.bfloat16).to(d)
    bias = torch.randn(272, generator=g).to(torch.bfloat16)
    for form, group, apply in (("block", 128, linear.apply_fp8_block), ("mx", 32, linear.apply_mxfp8)):
        _, w, _, ws = _operands(form, 1, 272, 512, g)
        out = apply(x, w.to(d), ws.to(d), bias.to(d))
        assert out.shape == (2, 20, 272) and linear.apply_mxfp8_fake(x, w, ws, bias).shape == (2, 20, 272)
        q, s = ops().per_token_group_quant_fp8(x.reshape(-1, 512), group, scale_ue8m0=True, scale_dtype=E8)
        qb, sb = q.cpu(), s.view(torch.uint8).cpu()
        assert_gemm_close(out.reshape(-1, 272), _ref(form, qb, w, sb, ws, torch.bfloat16, bias), f"apply {form}",
                          max_frac=0.03)
        q2, s2 = torch.empty_like(q), torch.empty_like(s)
        torch.ops._C.per_token_group_fp8_quant(x.reshape(-1, 512), q2, s2, group, 1e-10, -448.0, 448.0, True)
        assert_bit_exact(q2.view(torch.uint8), q.view(torch.uint8), "_C quantiser q")
        assert_bit_exact(s2.view(torch.uint8), s.view(torch.uint8), "_C quantiser s")
        out2, route = _run(qb, w, sb, ws, bias, torch.bfloat16, op=torch.ops._C.cutlass_scaled_mm)
        assert route == STREAM
        assert_bit_exact(out2, out.reshape(-1, 272), "_C cutlass_scaled_mm")


@pytest.mark.parametrize("form", ["block", "mx"])
def test_graph_replay_of_the_slab_path(form):
    """The K-split call captured into a HIP graph: three replays give the eager call's bits (nothing in the slab path
    depends on a memset or on what an earlier launch left in the workspace)."""
    m, n, k = 64, 1280, 8192
    d = dev()
    a, b_nk, a_s, b_s = _operands(form, m, n, k, torch.Generator().manual_seed(4))
    a, b, a_s, b_s = a.to(d), b_nk.to(d).t(), a_s.to(d).view(E8), b_s.to(d).view(E8).t()
    eager = torch.empty(m, n, dtype=torch.bfloat16, device=d)
    ops().cutlass_scaled_mm(eager, a, b, a_s, b_s, None)
    assert ops().scaled_mm_fp8_e8m0_last_route() == STREAM | SLABS
    out = torch.empty_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops().cutlass_scaled_mm(out, a, b, a_s, b_s, None)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops().cutlass_scaled_mm(out, a, b, a_s, b_s, None)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert_bit_exact(out, eager, "graph replay")


def test_argument_errors_and_untouched_paths():
    d = dev()
    out = torch.empty(16, 256, dtype=torch.bfloat16, device=d)
    f8 = lambda *shape: torch.zeros(*shape, dtype=F8, device=d)                            # noqa: E731
    e8 = lambda *shape: torch.full(shape, 127, dtype=torch.uint8, device=d).view(E8)       # noqa: E731
    f32 = lambda *shape: torch.ones(*shape, device=d)                                      # noqa: E731
    a, b = f8(16, 256), f8(256, 256).t()
    for mm in (ops().cutlass_scaled_mm, torch.ops._C.cutlass_scaled_mm):
        with pytest.raises(RuntimeError):                     # one fp32 and one E8M0 scale tensor
            mm(out, a, b, f32(16, 2), e8(2, 2).t(), None)
        with pytest.raises(RuntimeError):                     # k % 128 != 0
            mm(out, f8(16, 160), f8(256, 160).t(), e8(16, 5), e8(256, 5).t(), None)
        with pytest.raises(RuntimeError):                     # a scale shape off by one group
            mm(out, a, b, e8(16, 9), e8(256, 8).t(), None)
        with pytest.raises(RuntimeError):                     # MX b_scales not contiguous along the K groups
            mm(out, a, b, e8(16, 8), e8(8, 256), None)
        with pytest.raises(RuntimeError):                     # int8 operands
            mm(out, a.view(torch.int8), b.view(torch.int8), e8(16, 2), e8(2, 2).t(), None)
    x = torch.zeros(4, 256, dtype=torch.bfloat16, device=d)
    with pytest.raises(RuntimeError, match="only 128"):       # group 32 is for UE8M0 scales only
        ops().per_token_group_quant_fp8(x, 32)
    with pytest.raises(RuntimeError):                         # byte scales without the flag
        ops().per_token_group_quant_fp8(x, 128, scale_dtype=E8)
    q = torch.empty(4, 256, dtype=F8, device=d)
    with pytest.raises(RuntimeError):
        torch.ops._C.per_token_group_fp8_quant(x, q, f32(4, 8), 32, 1e-10, -448.0, 448.0, False)
    with pytest.raises(RuntimeError):
        torch.ops._C.per_token_group_fp8_quant(x, q, e8(4, 2), 128, 1e-10, -448.0, 448.0, False)
    # afterwards an fp32-scaled block call reports its route where it always did; the same call with byte scales
    # reports on the new query and leaves the fp32 entry's mask as it was
    ops().cutlass_scaled_mm(out, a, b, f32(16, 2), f32(2, 2), None)
    assert ops().scaled_mm_block_last_route() == 1 and float(out.float().abs().max()) == 0
    ops().cutlass_scaled_mm(out, a, b, e8(16, 2), e8(2, 2).t(), None)
    assert ops().scaled_mm_fp8_e8m0_last_route() == STREAM and ops().scaled_mm_block_last_route() == 1
