"""Micro-benchmark of paged prefill attention over head sizes: bf16, 8 sequences x 1024 new tokens (context 0) and
8 x 512 new tokens on 512 of context, (heads, kv heads, head size) = (32, 8, 64), (16, 8, 256) and, as the yardstick,
(32, 8, 128).  A CUDA graph of 30 launches over rotating cache copies, best of 5 replays
(a kernel that needs more than 5 ms per launch: best of 3 single launches); us per launch and TFLOP/s
(4 * head_size FLOPs per visible (query, key) pair and head).  Run on the GPU box.
usage: bench_prefill_attn.py [--ab LIB.so]  (--ab: also run the same benchmark in a child process against another
build of the library, e.g. one of the parent commit, 3 alternating rounds)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--ab" in sys.argv:
    other = sys.argv[sys.argv.index("--ab") + 1]
    for r in range(3):
        for tag, env in (("new", {}), ("old", {"MI355X_HOTPATH_LIB": os.path.join(ROOT, other)})):
            out = subprocess.run([sys.executable, __file__], env=dict(os.environ, **env), capture_output=True, text=True)
            for line in out.stdout.splitlines():
                print(f"[{tag} round {r}] {line}", flush=True)
            if out.returncode:
                print(out.stderr[-2000:])
    sys.exit(0)
import ctypes
import torch
from vllm_metax_amd import _abi
if os.environ.get("MI355X_HOTPATH_LIB"):   # an older build has no route diagnostic (not used here): do not bind it
    if not hasattr(ctypes.CDLL(os.environ["MI355X_HOTPATH_LIB"]), "mi355x_paged_prefill_last_route"):
        _abi.PROTOTYPES.pop("mi355x_paged_prefill_last_route")
from vllm_metax_amd import _custom_ops as ops
d = torch.device("cuda:0")
S, BS, copies, reps = 8, 16, 3, 30
dt = torch.bfloat16
for new, ctx in ((1024, 0), (512, 512)):
    L = new + ctx
    nblk = L // BS
    nb = S * nblk
    for H, KVH, D in ((32, 8, 64), (16, 8, 256), (32, 8, 128)):
        kcs = [(torch.randn(nb, KVH, D // 8, BS, 8, device=d) * 0.3).to(dt) for _ in range(copies)]
        vcs = [(torch.randn(nb, KVH, D, BS, device=d) * 0.3).to(dt) for _ in range(copies)]
        q = (torch.randn(S * new, H, D, device=d) * 0.5).to(dt)
        out = torch.empty_like(q)
        bt = torch.randperm(nb, device=d).to(torch.int32).view(S, nblk)
        sl = torch.full((S,), L, device=d, dtype=torch.int32)
        cu = torch.arange(S + 1, device=d, dtype=torch.int32) * new
        def fn(i): ops.paged_prefill_attention(out, q, kcs[i % copies], vcs[i % copies], KVH, D ** -0.5, bt, sl, cu, new, BS)
        def timed(run, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); run(); b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / n
        fn(0)
        how = ""
        if timed(lambda: fn(1), 1) > 5e3:
            # the general kernel at these shapes takes tens of milliseconds and more: single launches, best of 3
            best, how = min(timed(lambda: fn(i), 1) for i in range(3)), "  (single launches)"
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(reps): fn(i)
            g.replay(); torch.cuda.synchronize()
            best = min(timed(g.replay, reps) for _ in range(5))
        pairs = S * H * (new * ctx + new * (new + 1) // 2)       # visible (query, key) pairs over all heads
        print(f"new={new} ctx={ctx} heads={H}/{KVH} d={D}: {best:9.1f} us per launch  {4 * D * pairs / best / 1e6:7.1f} TFLOP/s{how}",
              flush=True)
