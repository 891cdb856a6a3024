"""Micro-benchmark of the E8M0-scaled fp8 GEMM (fp8_e8m0_gemm.hip), block form and MX form, against the two paths a
ue8m0 user has without it, in the same process at the same (m, n, k): the fp32 block-scaled path (fp8_block_gemm.hip)
and the row-scaled fp8 cutlass_scaled_mm (the floor: same operand bytes, same MFMAs).  One TP = 8 rank of Llama-3-70B
(the shapes of scripts/bench_fp8_block.py) at M = 64 / 2048, and with --8b the Llama-3-8B layer shapes at M = 64 / 576 /
2048; bf16 output.  A CUDA graph of 30 launches over 3 rotating weight copies, best of 5 replays; us per launch, the
routes, the ratios.  The four paths alternate inside every (shape, m), and --repeat N runs the whole table N times:
the spread between repeats is the noise a difference has to exceed.
--threshold: M = 64 .. 448 with every call forced to the stream kernel (passes of 64 rows) and to the tile kernel
(MI355X_F8E_TILE_MIN_M, read once per process: two child processes), the measurement the router's threshold rests on.
Run on the GPU box."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--threshold" in sys.argv:
    for tag, min_m in (("stream passes", "100000"), ("tile kernel", "1")):
        out = subprocess.run([sys.executable, __file__, "--ms", "64,128,192,256,320,384,448", "--e8m0-only"],
                             env=dict(os.environ, MI355X_F8E_TILE_MIN_M=min_m), capture_output=True, text=True)
        for line in out.stdout.splitlines():
            print(f"[{tag}] {line}", flush=True)
        if out.returncode:
            print(out.stderr[-2000:])
            sys.exit(out.returncode)
    sys.exit(0)
import torch
from vllm_metax_amd import _custom_ops as ops
d = torch.device("cuda:0")
FP8, E8, copies, reps = torch.float8_e4m3fn, torch.float8_e8m0fnu, 3, 30
if "--8b" in sys.argv:
    SHAPES = (("qkv", 4096, 6144), ("o", 4096, 4096), ("gate_up", 4096, 28672), ("down", 14336, 4096))
    MS = [64, 576, 2048]
else:
    SHAPES = (("qkv", 8192, 1280), ("o", 1024, 8192), ("gate_up", 8192, 7168), ("down", 3584, 8192))
    MS = [64, 2048]
if "--ms" in sys.argv:
    MS = [int(v) for v in sys.argv[sys.argv.index("--ms") + 1].split(",")]
REPEAT = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 1
E8_ONLY = "--e8m0-only" in sys.argv


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


def rand_scales(*shape):
    return torch.randint(121, 127, shape, dtype=torch.uint8, device=d).view(E8)


for rep in range(REPEAT):
    for name, k, n in SHAPES:
        nb, kb = (n + 127) // 128, k // 128
        w8 = [(torch.randn(n, k, device=d) * 2).to(FP8).t() for _ in range(copies)]
        sb_blk, sb_mx = rand_scales(nb, kb).t(), rand_scales(n, k // 32).t()
        sb_f32, bs_col = torch.rand(nb, kb, device=d).t() * 9e-3 + 1e-3, torch.rand(1, n, device=d) * 9e-3 + 1e-3
        for m in MS:
            a8 = (torch.randn(m, k, device=d) * 2).to(FP8)
            sa_blk, sa_mx = rand_scales(m, kb), rand_scales(m, k // 32)
            sa_f32, as_row = torch.rand(m, kb, device=d) * 9e-3 + 1e-3, torch.rand(m, 1, device=d) * 9e-3 + 1e-3
            out = torch.empty(m, n, dtype=torch.bfloat16, device=d)
            tb = bench(lambda i: ops.cutlass_scaled_mm(out, a8, w8[i % copies], sa_blk, sb_blk, None))
            route = ops.scaled_mm_fp8_e8m0_last_route()
            tm = bench(lambda i: ops.cutlass_scaled_mm(out, a8, w8[i % copies], sa_mx, sb_mx, None))
            line = f"{name:8s} k={k} n={n} m={m:4d}: e8m0 block {tb:8.1f} us   mx {tm:8.1f} us (route {route})"
            if not E8_ONLY:
                tf = bench(lambda i: ops.cutlass_scaled_mm(out, a8, w8[i % copies], sa_f32, sb_f32, None))
                tr = bench(lambda i: ops.cutlass_scaled_mm(out, a8, w8[i % copies], as_row, bs_col, None))
                line += (f"   fp32 block {tf:8.1f} us (route {ops.scaled_mm_block_last_route()})   row-scaled {tr:8.1f} us"
                         f"   block/fp32-block {tb / tf:.3f}   block/row {tb / tr:.3f}   mx/row {tm / tr:.3f}")
            nbytes = (n + m) * k + m * kb + nb * kb + 2 * m * n
            print(line + f"   {nbytes / tb / 8e6 * 100:5.1f} % of 8 TB/s   {2.0 * m * n * k / tb / 1e6:7.1f} TFLOP/s",
                  flush=True)
