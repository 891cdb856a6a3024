"""Micro-benchmark of the MX-FP4 GEMM (mxfp4_gemm.hip) against the row-scaled fp8 cutlass_scaled_mm at the same
(m, n, k): the stream kernel reads 0.53 x the fp8 weight bytes and issues half the MFMAs, so the fp8 time is the
ceiling.  One TP = 8 rank of Llama-3-70B (the shapes of scripts/bench_fp8_block.py), bf16 output.  A CUDA graph of 30
launches over 3 rotating weight copies, best of 5 replays; us per launch, the route, the stream kernel's share of
8 TB/s against the algorithmic bytes (weights + their scales + activations + output) and TFLOP/s.
--threshold: M = 64 .. 384 with every call forced to the stream kernel (passes of 64 rows) and to the tile kernel
(MI355X_MX4_TILE_MIN_M, read once per process: two child processes), the measurement the router's threshold rests on.
Run on the GPU box."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--threshold" in sys.argv:
    for tag, min_m in (("stream passes", "100000"), ("tile kernel", "1")):
        out = subprocess.run([sys.executable, __file__, "--ms", "64,65,96,128,192,256,320,384"],
                             env=dict(os.environ, MI355X_MX4_TILE_MIN_M=min_m), capture_output=True, text=True)
        for line in out.stdout.splitlines():
            print(f"[{tag}] {line}", flush=True)
        if out.returncode:
            print(out.stderr[-2000:])
            sys.exit(out.returncode)
    sys.exit(0)
import torch
from vllm_metax_amd import _custom_ops as ops
d = torch.device("cuda:0")
FP8, F4, E8, copies, reps = torch.float8_e4m3fn, torch.float4_e2m1fn_x2, torch.float8_e8m0fnu, 3, 30
SHAPES = (("qkv", 8192, 1280), ("o", 1024, 8192), ("gate_up", 8192, 7168), ("down", 3584, 8192))
MS = [int(v) for v in sys.argv[sys.argv.index("--ms") + 1].split(",")] if "--ms" in sys.argv else [1, 16, 64, 2048]


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


def rand_bytes(*shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=d)


def rand_scales(*shape):
    return torch.randint(121, 127, shape, dtype=torch.uint8, device=d).view(E8)


for name, k, n in SHAPES:
    w4 = [rand_bytes(n, k // 2).view(F4).t() for _ in range(copies)]
    s4 = rand_scales(n, k // 32).t()
    w8 = [(torch.randn(n, k, device=d) * 2).to(FP8).t() for _ in range(copies)]
    bs_col = torch.rand(1, n, device=d) * 9e-3 + 1e-3
    for m in MS:
        a4, as4 = rand_bytes(m, k // 2).view(F4), rand_scales(m, k // 32)
        a8 = (torch.randn(m, k, device=d) * 2).to(FP8)
        as_row = torch.rand(m, 1, device=d) * 9e-3 + 1e-3
        out = torch.empty(m, n, dtype=torch.bfloat16, device=d)
        t4 = bench(lambda i: ops.cutlass_scaled_mm(out, a4, w4[i % copies], as4, s4, None))
        route = ops.scaled_mm_mxfp4_last_route()
        t8 = bench(lambda i: ops.cutlass_scaled_mm(out, a8, w8[i % copies], as_row, bs_col, None))
        nbytes = (n + m) * (k // 2 + k // 32) + 2 * m * n
        print(f"{name:8s} k={k} n={n} m={m:4d}: mxfp4 {t4:8.1f} us (route {route})   fp8 row-scaled {t8:8.1f} us"
              f"   ratio {t4 / t8:.3f}   {nbytes / t4 / 8e6 * 100:5.1f} % of 8 TB/s   "
              f"{2.0 * m * n * k / t4 / 1e6:7.1f} TFLOP/s", flush=True)
