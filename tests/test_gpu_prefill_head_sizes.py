"""GPU parity: the MFMA prefill kernel of head sizes 64 and 256 (csrc/prefill_attention_hd.hip) against the CPU oracle.

Every case asserts the route (paged_prefill_last_route): the general kernel serves these shapes too, so the tolerance
alone would not tell which kernel ran.  Bounds are those of the operation's other tests: 16-bit cache as
tests/test_gpu_prefill_attention.py (2e-3 * max|ref| + one output ulp at max|ref|), fp8 cache as
tests/test_gpu_fp8_kv.py::test_paged_prefill_fp8kv.  Cache tails are poisoned with NaN and `out` starts as NaN.
"""
import numpy as np
import pytest
import torch

from tests.test_cpu_ref_fixtures import close_to_f32
from tests.util import assert_bit_exact, assert_close_rel, dev, make_kv_cache_x

pytestmark = pytest.mark.gpu

from oracle import ref_ops as R  # noqa: E402

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
EPS = {F16: 2.0 ** -10, BF: 2.0 ** -7, F32: 2.0 ** -23}
H, KVH = 8, 2
MIXED = ([130, 7, 64], [130, 300, 64])                # pure prefill + chunked (context > 0), varlen
# the same and 29 decode-like rows: 32 sequences x 2 query blocks x 8 heads = 512 workgroups, from where on head size
# 64 runs 128 query rows per workgroup (every smaller grid here runs 64)
WIDE = (MIXED[0] + [1] * 29, MIXED[1] + [33] * 29)


def ops():
    from vllm_metax_amd import _custom_ops
    return _custom_ops


def _run(spec, D, dtype, route, bs=16, window=None, softcap=None, fp8=None):
    """fp8: None (cache of `dtype`), "fp8" (e4m3) or "fp8_e5m2", with (k_scale, v_scale) = (0.5, 1.7)."""
    q_lens, seq_lens = spec
    torch.manual_seed(7)
    S = len(q_lens)
    mb = (max(seq_lens) + bs - 1) // bs
    nb = S * mb + 5
    bt = torch.randperm(nb)[:S * mb].to(torch.int32).reshape(S, mb)
    cu = torch.zeros(S + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(q_lens).cumsum(0)
    sl = torch.tensor(seq_lens, dtype=torch.int32)
    scale = D ** -0.5
    d = dev()
    ks = vs = None
    if fp8 is None:
        kc, vc = make_kv_cache_x(nb, bs, KVH, D, dtype, 7)
        q = (torch.randn(int(cu[-1]), H, D) * (2.0 if softcap else 0.5)).to(dtype)   # x4: the cap must bite
        ref = R.paged_prefill_attention(q, kc, vc, KVH, scale, bt, sl, cu, window, softcap)
        poison = float("nan")
    else:
        fmt, name = (torch.float8_e5m2, "e5m2") if fp8 == "fp8_e5m2" else (torch.float8_e4m3fn, "e4m3")
        kc = (torch.rand(nb, KVH, D // 16, bs, 16) * 2 - 1).to(fmt).view(torch.uint8)
        vc = (torch.rand(nb, KVH, D, bs) * 2 - 1).to(fmt).view(torch.uint8)
        q = (torch.randn(int(cu[-1]), H, D) * 0.7).to(dtype)
        ref = R.paged_prefill_attention(q, R.fp8_dequant(kc, 0.5, dtype, name), R.fp8_dequant(vc, 1.7, dtype, name),
                                        KVH, scale, bt, sl, cu)
        poison = 0x7f                                  # NaN in both byte formats
        ks, vs = (torch.tensor([x], dtype=F32, device=d) for x in (0.5, 1.7))
    for s, L in enumerate(seq_lens):
        if L % bs:
            blk = int(bt[s, (L - 1) // bs])
            kc[blk, :, :, L % bs:, :] = poison
            vc[blk, :, :, L % bs:] = poison
    out = torch.full(q.shape, float("nan"), dtype=dtype, device=d)
    ops().paged_prefill_attention(out, q.to(d), kc.to(d), vc.to(d), KVH, scale, bt.to(d), sl.to(d), cu.to(d),
                                  max(q_lens), bs, fp8 or "auto", ks, vs, window, softcap)
    torch.cuda.synchronize()
    assert ops().paged_prefill_last_route() == route
    if fp8 is None:
        assert_close_rel(out, ref, 2e-3, f"prefill d{D}", abs_floor=EPS[dtype] * ref.float().abs().max().item())
    else:
        close_to_f32(out.cpu(), ref.float(), f"prefill {fp8} d{D}", rel=2e-3 + 2.0 ** -8)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("spec", [
    ([1], [1]), ([17], [40]),                         # one row; a partial query tile
    ([129], [129]),                                   # tile boundary + 1
    MIXED,                                            # contexts that end mid-stage (32- and 64-key stages)
    ([32, 1, 200], [1100, 77, 200]),                  # 69 blocks: the block-table register is refilled; decode-like row
    WIDE,
])
def test_prefill_hd_plain(dtype, D, spec):
    _run(spec, D, dtype, ops().PF_ROUTE_HD)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("window,softcap", [(1, None), (17, None), (256, 50.0), (None, 50.0)])
@pytest.mark.parametrize("spec", [MIXED, ([300], [813]), WIDE])
def test_prefill_hd_window_softcap(dtype, D, window, softcap, spec):
    _run(spec, D, dtype, ops().PF_ROUTE_HD, window=window, softcap=softcap)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("fp8", ["fp8", "fp8_e5m2"])
@pytest.mark.parametrize("spec", [([17], [40]), MIXED, WIDE])
def test_prefill_hd_fp8_kv(dtype, D, fp8, spec):
    _run(spec, D, dtype, ops().PF_ROUTE_HD, fp8=fp8)


def test_prefill_routing_edges():
    """What the head-size kernel must not take: another block size, head size 128, fp32."""
    spec = ([9, 33], [20, 33])
    _run(spec, 64, BF, ops().PF_ROUTE_GENERIC, bs=32)
    _run(spec, 128, BF, ops().PF_ROUTE_D128)
    _run(spec, 64, F32, ops().PF_ROUTE_GENERIC)


def test_backend_mixed_batch_head_64():
    """paged_attention_forward on 2 decode rows + 2 prefill rows at head size 64: the prefill rows reach the new kernel
    through the backend (metadata as tests/test_gpu_golden_backend.py::test_backend_mixed_batches)."""
    from vllm_metax_amd.attention import backend as B
    torch.manual_seed(0)
    D, bs, dt = 64, 16, BF
    q_lens, seq_lens = [1, 1, 8, 130], [40, 513, 100, 300]
    n = len(q_lens)
    mb = (max(seq_lens) + bs - 1) // bs
    nb = n * mb + 2
    d = dev()
    kc, vc = B.split_kv_cache(torch.zeros(B.kv_cache_shape(nb, bs, KVH, D), dtype=dt), KVH, D)
    kc, vc = kc.contiguous(), vc.contiguous()
    bt = torch.randperm(nb)[:n * mb].to(torch.int32).reshape(n, mb)

    def slots_of(r, lo, hi):
        pos = torch.arange(lo, hi)
        return bt[r, pos // bs].long() * bs + pos % bs
    for r in range(n):                                 # the context of every request
        ctx = seq_lens[r] - q_lens[r]
        R.reshape_and_cache((torch.randn(ctx, KVH, D) * 0.3).to(dt), (torch.randn(ctx, KVH, D) * 0.3).to(dt), kc, vc,
                            slots_of(r, 0, ctx))
    T = sum(q_lens)
    qsl = torch.tensor([0] + list(np.cumsum(q_lens)), dtype=torch.int32)
    q, k, v = ((torch.randn(T, h, D) * 0.3).to(dt) for h in (H, KVH, KVH))
    slots = torch.cat([slots_of(r, seq_lens[r] - q_lens[r], seq_lens[r]) for r in range(n)])
    kvd = torch.stack([kc.reshape(nb, -1), vc.reshape(nb, -1)]).to(d)
    R.reshape_and_cache(k, v, kc, vc, slots)
    slt = torch.tensor(seq_lens, dtype=torch.int32)
    ref = R.paged_prefill_attention(q, kc, vc, KVH, D ** -0.5, bt, slt, qsl)
    md = B.build_metadata(qsl.to(d), qsl.tolist(), slt.to(d), seq_lens, bt.to(d), slots.to(d), T, max(q_lens),
                          max(seq_lens), H, D, dt)
    out = torch.zeros(T, H, D, dtype=dt, device=d)
    B.paged_attention_forward(q.to(d), k.to(d), v.to(d), kvd, md, out, KVH, D ** -0.5)
    assert ops().paged_prefill_last_route() == ops().PF_ROUTE_HD
    assert_bit_exact(B.split_kv_cache(kvd, KVH, D)[0].contiguous(), kc, "key cache after write")
    assert_close_rel(out, ref, 2e-3, "backend output", abs_floor=EPS[dt] * ref.float().abs().max().item())
