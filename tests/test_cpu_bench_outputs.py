"""CPU: bench.py's option surface and `--dump-outputs` writer (no GPU: the writer is fed a stand-in model)."""
import importlib.util
import pathlib
import sys
import types

import numpy as np
import torch

BENCH = pathlib.Path(__file__).resolve().parents[1] / "bench.py"


def _bench():
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _model(vocab=1000):
    g = torch.Generator().manual_seed(0)
    return types.SimpleNamespace(
        job_first_tokens=torch.randint(0, vocab, (6,), generator=g),
        d_tokens=torch.randint(0, vocab, (6,), generator=g),
        d_positions=torch.arange(6) + 2 ** 40,            # int64 beyond float32's integers: float64 keeps them
        last_prefill_logits=torch.randn(2, vocab, generator=g).to(torch.bfloat16),
        last_logits=torch.randn(6, vocab, generator=g).to(torch.bfloat16))


def test_plain_run_is_the_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_arrays(tmp_path):
    bench, m = _bench(), _model()
    info = bench.dump_outputs(m, str(tmp_path / "out"))
    files = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert files == ["final_positions.npy", "final_tokens.npy", "first_tokens.npy", "last_decode_logits.npy",
                     "last_prefill_logits.npy"]
    for name, t in (("first_tokens", m.job_first_tokens), ("final_tokens", m.d_tokens),
                    ("final_positions", m.d_positions), ("last_prefill_logits", m.last_prefill_logits),
                    ("last_decode_logits", m.last_logits)):
        a = np.load(tmp_path / "out" / (name + ".npy"))
        assert a.dtype == (np.float32 if "logits" in name else np.float64)
        assert a.shape == tuple(t.shape) and info[name] == {"shape": list(t.shape), "stored": t.numel()}
        assert np.array_equal(a, t.to(torch.float64).numpy())       # bf16 -> float32 and int64 -> float64: exact here


def test_dump_outputs_samples_what_exceeds_the_limit(tmp_path, monkeypatch):
    bench, m = _bench(), _model()
    small = 3 * 6 * 8 + 2 * 1000 * 4        # the three integer arrays and the prefill logits fit whole ...
    limit = small + 1001 * 4                # ... and 1001 of the 6000 decode logits
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    runs = []
    for d in ("a", "b"):
        info = bench.dump_outputs(m, str(tmp_path / d))
        runs.append({p.name: np.load(p) for p in (tmp_path / d).iterdir()})
        assert sum(v.nbytes for v in runs[-1].values()) == limit
    assert info["last_decode_logits"] == {"shape": [6, 1000], "stored": 1001}
    assert info["last_prefill_logits"]["stored"] == 2000
    a, b = runs[0]["last_decode_logits.npy"], runs[1]["last_decode_logits.npy"]
    assert a.shape == (1001,) and np.array_equal(a, b)              # the same sample every time
    idx = np.sort(np.random.default_rng(0).choice(6000, size=1001, replace=False))
    assert np.array_equal(a, m.last_logits.float().numpy().reshape(-1)[idx])
