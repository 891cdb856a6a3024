"""GPU: bench.py's command line on the tiny model — what a plain run does and leaves out, what `--full` adds,
`--steps` / `ms_per_step` / `value` agree, `--dump-outputs` writes the last job's outputs.  (The benchmark is
started as a process because its command line is what is tested.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, LIN, LOUT = 4, 64, 8
JOB = ["--gpus", "1", "--model", "tiny", "--batch", str(B), "--input-len", str(LIN), "--output-len", str(LOUT),
       "--chunk-seqs", "2"]


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *JOB, *extra], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def _check_headline(r, steps, warmup):
    assert (r["steps"], r["warmup"], r["unit"], r["higher_is_better"], r["dtype"]) == \
        (steps, warmup, "output tokens/s", True, "bf16")
    assert r["metric"].startswith("output tokens/sec (") and r["ms_per_step"] > 0
    # value = tokens of the timed jobs / their time; ms_per_step = that time / steps (both rounded on the line)
    assert r["value"] == pytest.approx(B * LOUT / (r["ms_per_step"] * 1e-3), rel=1e-3)
    assert r["config"]["outputs_finite"] and r["config"]["decode_graph"]


def test_plain_run_times_the_jobs_and_dumps_their_outputs(tmp_path):
    out = tmp_path / "dump"
    r = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    _check_headline(r, 3, 1)
    assert r["full"] is False and r["roofline"] is None and r["roofline_other"] == []
    assert not {"cpu_baseline", "plugin_surface", "dp_replicas", "baseline_tp8_model"} & set(r)
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["final_positions", "final_tokens", "first_tokens", "last_decode_logits",
                           "last_prefill_logits"]
    vocab = got["last_decode_logits"].shape[1]
    assert got["last_decode_logits"].shape == (B, vocab) and got["last_prefill_logits"].shape == (2, vocab)
    for name in ("first_tokens", "final_tokens", "final_positions"):
        assert got[name].dtype == np.float64 and got[name].shape == (B,)
    for name in ("last_decode_logits", "last_prefill_logits"):
        assert got[name].dtype == np.float32 and np.isfinite(got[name]).all() and np.abs(got[name]).max() > 0
    assert (got["final_positions"] == LIN + LOUT - 1).all()
    # the dumped tokens are the greedy choice of the dumped logits: last chunk's first tokens, last step's tokens
    for tok, lg in ((got["first_tokens"][-2:], got["last_prefill_logits"]),
                    (got["final_tokens"], got["last_decode_logits"])):
        assert np.array_equal(lg[np.arange(len(tok)), tok.astype(np.int64)], lg.max(-1))
    assert r["dumped_outputs"]["last_decode_logits"] == {"shape": [B, vocab], "stored": B * vocab}


def test_full_run_adds_the_other_measurements():
    r = _bench("--steps", "2", "--warmup", "1", "--full", "--skip-cpu")
    _check_headline(r, 2, 1)
    assert r["full"] is True and r["roofline"]["kernel"] and len(r["roofline_other"]) > 0
    assert "error" not in r["plugin_surface"] and r["plugin_surface"]["value"] > 0
    assert "cpu_baseline" not in r and "dumped_outputs" not in r
