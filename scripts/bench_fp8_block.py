"""Micro-benchmark of the block-scaled fp8 GEMM (fp8_block_gemm.hip) against the row-scaled cutlass_scaled_mm at the
same shapes — the same bytes and the same MFMAs, so the row-scaled time is the floor.  One TP = 8 rank of Llama-3-70B
(the shapes of tests/test_gpu_fp8_gemm.py::test_scaled_mm_fp8_llama70b_tp8_shapes), bf16 output.  A CUDA graph of 30
launches over 3 rotating weight copies, best of 5 replays; us per launch and the route of the block call.
--threshold: M = 128 .. 512 with every call forced to the decode kernel (passes of 64 rows) and to the tile kernel
(MI355X_F8B_TILE_MIN_M, read once per process: two child processes), the measurement the router's threshold rests on.
Run on the GPU box."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--threshold" in sys.argv:
    for tag, min_m in (("decode passes", "100000"), ("tile kernel", "1")):
        out = subprocess.run([sys.executable, __file__, "--ms", "128,256,320,384,512"],
                             env=dict(os.environ, MI355X_F8B_TILE_MIN_M=min_m), capture_output=True, text=True)
        for line in out.stdout.splitlines():
            print(f"[{tag}] {line}", flush=True)
        if out.returncode:
            print(out.stderr[-2000:])
            sys.exit(out.returncode)
    sys.exit(0)
import torch
from vllm_metax_amd import _custom_ops as ops
d = torch.device("cuda:0")
FP8, copies, reps = torch.float8_e4m3fn, 3, 30
SHAPES = (("qkv", 8192, 1280), ("o", 1024, 8192), ("gate_up", 8192, 7168), ("down", 3584, 8192))
MS = [int(v) for v in sys.argv[sys.argv.index("--ms") + 1].split(",")] if "--ms" in sys.argv else [64, 2048]


def timed(run, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); run(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def bench(fn):
    fn(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(reps): fn(i)
    g.replay(); torch.cuda.synchronize()
    return min(timed(g.replay, reps) for _ in range(5))


for name, k, n in SHAPES:
    ws = [(torch.randn(n, k, device=d) * 2).to(FP8).t() for _ in range(copies)]
    bs_col = torch.rand(1, n, device=d) * 9e-3 + 1e-3
    bs_blk = (torch.rand((n + 127) // 128, k // 128, device=d) * 9e-3 + 1e-3).t()
    for m in MS:
        a = (torch.randn(m, k, device=d) * 2).to(FP8)
        as_row = torch.rand(m, 1, device=d) * 9e-3 + 1e-3
        as_grp = torch.rand(m, k // 128, device=d) * 9e-3 + 1e-3
        out = torch.empty(m, n, dtype=torch.bfloat16, device=d)
        t_blk = bench(lambda i: ops.cutlass_scaled_mm(out, a, ws[i % copies], as_grp, bs_blk, None))
        route = ops.scaled_mm_block_last_route()
        t_row = bench(lambda i: ops.cutlass_scaled_mm(out, a, ws[i % copies], as_row, bs_col, None))
        print(f"{name:8s} k={k} n={n} m={m:4d}: block {t_blk:8.1f} us (route {route})   row-scaled {t_row:8.1f} us"
              f"   ratio {t_blk / t_row:.3f}   block {2.0 * m * n * k / t_blk / 1e6:7.1f} TFLOP/s", flush=True)
