"""``bench.py`` as a plain run: only the headline is measured, ``--steps`` sets the timed steps,
and ``--dump-outputs`` writes, as float32 ``.npy`` files, one step of the timed path from the
seeded initial weights: the same arrays on every run, whatever the number of timed steps."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--warmup", "1", "--batch", "16", "--enc", "64", "--dec", "8", "--vocab", "2000",
         "--hidden", "64", "--emb", "64", "--pool", "2"]


def _run(capsys, extra):
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    assert bench.main(SMALL + extra) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only_and_dumps_outputs(capsys, tmp_path):
    import bench
    d = str(tmp_path / "out")
    rec = _run(capsys, ["--steps", "3", "--dump-outputs", d])
    assert rec["metric"] == "train_tokens_per_sec" and rec["unit"] == "tokens/s" and rec["dtype"] == "bf16"
    assert rec["higher_is_better"] is True and rec["steps"] == 3
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # nothing beside the headline ran
    assert not [k for k in rec if k.startswith(("beam4_", "config5_"))]
    assert "phase_ms_max_over_ranks" not in rec["config"]
    names = sorted(os.listdir(d))
    assert names == ["coverage_loss.npy", "global_norm.npy", "grad_sample.npy", "loss.npy", "params_sample.npy",
                     "total_loss.npy"]
    total = 0
    for n in names:
        a = np.load(os.path.join(d, n))
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    one = {n: float(np.load(os.path.join(d, n + ".npy"))[0]) for n in ("loss", "coverage_loss", "total_loss")}
    assert one["total_loss"] == pytest.approx(one["loss"] + one["coverage_loss"], rel=1e-6)  # cov_loss_wt = 1
    n_par = len(np.load(os.path.join(d, "params_sample.npy")))
    assert 0 < n_par <= bench.DUMP_SAMPLE and len(np.load(os.path.join(d, "grad_sample.npy"))) == n_par
    assert np.abs(np.load(os.path.join(d, "grad_sample.npy"))).max() > 0


def test_dumped_outputs_repeat_from_run_to_run(capsys, tmp_path):
    """Same arguments, same arrays.  The dumped step starts from the seeded weights, so two runs
    differ only in the order of the fp32 atomic gradient sums: around fp32 epsilon (6e-8) in
    relative norm, and at most an isolated flipped bf16 rounding (2^-8 on single elements of an
    intermediate), far below the bound of 1e-4.  State carried through the timed steps instead
    diverges past that bound within 5 steps at the benchmark's shape (bench.dump_step)."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _run(capsys, ["--steps", "4", "--dump-outputs", a])
    _run(capsys, ["--steps", "4", "--dump-outputs", b])
    for n in sorted(os.listdir(a)):
        x, y = np.load(os.path.join(a, n)).astype(np.float64), np.load(os.path.join(b, n)).astype(np.float64)
        rel = np.linalg.norm(x - y) / np.linalg.norm(x)
        print(n, "relative difference", rel)
        assert rel <= 1e-4, (n, rel)


def test_full_run_adds_phase_times_and_decode(capsys):
    rec = _run(capsys, ["--steps", "2", "--full", "--decode-batches", "2", "--decode-articles", "8",
                        "--config5-steps", "0"])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert rec["beam4_summaries_per_sec"] > 0
    assert set(rec["config"]["phase_ms_max_over_ranks"]) >= {"ms_fwd_head", "ms_optimizer"}
