"""Micro-benchmark of the 8-bit GPTQ GEMM below 1024 rows (w8a16_gemm_stream_kernel): one TP = 8 rank of Qwen2-72B,
bf16, group 128, M = 1, 16, 64, 256, 512.  A CUDA graph of 30 launches over rotating weight copies, best of 5 replays
(a call that needs more than 5 ms: best of 3 single launches); us per launch, achieved fraction of 8 TB/s against the
algorithmic bytes N K + (N K / g)(sizeof(T) + 1) + 2 M K + 2 M N, and the 4-bit GEMM at the same shape as a yardstick.
--sweep: every forced (k-parts, K split) of the stream kernel next to the planner's choice (MI355X_W8_STREAM_FORCE).
--ab LIB.so: the default table once more in a child process against another build of the library (the parent's).
Run on the GPU box."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--ab" in sys.argv:
    other = sys.argv[sys.argv.index("--ab") + 1]
    for tag, env in (("new", {}), ("old", {"MI355X_HOTPATH_LIB": os.path.join(ROOT, other)})):
        out = subprocess.run([sys.executable, __file__], env=dict(os.environ, **env), capture_output=True, text=True)
        for line in out.stdout.splitlines():
            print(f"[{tag}] {line}", flush=True)
        if out.returncode:
            print(out.stderr[-2000:])
    sys.exit(0)
import torch
from vllm_metax_amd import _custom_ops as ops
d = torch.device("cuda:0")
dt, group, copies, reps = torch.bfloat16, 128, 3, 30
SHAPES = (("qkv", 8192, 1280), ("o", 1024, 8192), ("gate_up", 8192, 7424), ("down", 3712, 8192))
none = torch.empty(0, dtype=torch.int32, device=d)


def timed(run, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); run(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def bench(fn):
    fn(0)
    if timed(lambda: fn(1), 1) > 5e3:
        return min(timed(lambda: fn(i), 1) for i in range(3))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(reps): fn(i)
    g.replay(); torch.cuda.synchronize()
    return min(timed(g.replay, reps) for _ in range(5))


def weights(k, n, bit):
    per = 32 // bit
    return [(torch.randint(-2 ** 31, 2 ** 31 - 1, (k // per, n), device=d, dtype=torch.int32),
             torch.randint(-2 ** 31, 2 ** 31 - 1, (k // group, n // per), device=d, dtype=torch.int32),
             (torch.rand(k // group, n, device=d) * 4e-4 + 1e-4).to(dt)) for _ in range(copies)]


for name, k, n in SHAPES:
    w8, w4 = weights(k, n, 8), weights(k, n, 4)
    for m in (1, 16, 64, 256, 512):
        x = (torch.randn(m, k, device=d) * 0.5).to(dt)
        def gemm(ws, bit): return lambda i: ops.gptq_gemm(x, *ws[i % copies][:2], ws[i % copies][2], none, True, bit, group, none, none, True)
        os.environ.pop("MI355X_W8_STREAM_FORCE", None)
        t8 = bench(gemm(w8, 8))
        route = ops.w4a16_last_route()
        t4 = bench(gemm(w4, 4))
        nbytes = n * k + (n * k // group) * 3 + 2 * m * k + 2 * m * n
        print(f"{name:8s} k={k} n={n} m={m:3d}: 8-bit {t8:9.1f} us (route {route:3d}, {nbytes / t8 / 8e6:5.1%} of 8 TB/s)"
              f"   4-bit {t4:7.1f} us", flush=True)
        if "--sweep" in sys.argv:
            res = {}
            for kw in (1, 2, 4):
                for sk in (1, 2, 4, 8):
                    os.environ["MI355X_W8_STREAM_FORCE"] = f"{kw},{sk}"
                    res[kw, sk] = bench(gemm(w8, 8))
            os.environ.pop("MI355X_W8_STREAM_FORCE", None)
            best = min(res, key=res.get)
            print("    sweep (kw,sk: us) " + " ".join(f"{a},{b}:{t:.1f}" for (a, b), t in res.items()))
            print(f"    best forced {best[0]},{best[1]} {res[best]:.1f} us; planner {t8:.1f} us = {t8 / res[best]:.3f} x best", flush=True)
