"""CPU: the decision logic of bench.py (benchkit/ranks.py, benchkit/report.py) that cannot wait for an 8-GPU box to be exercised
for the first time.

* `measure_exchange_schedules`: a failure while capturing the OPTIONAL second exchange schedule must leave the first
  schedule's finished graph-replayed measurement standing -- mocked captures, no GPU.
* `counters_current` / scripts/lib_identity.py: committed counter passes are quoted only for the library they were taken on.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402  (re-exports the pieces below)
from benchkit import ranks as bench_ranks, report as bench_report  # noqa: E402


class _Clock:
    """time_region(run, n) -> n * the per-step time the mocked replay callable stands for."""

    def __init__(self):
        self.calls = []

    def __call__(self, run, n):
        self.calls.append((run.__name__, n))
        return n * run()


def _schedules(ms_a, ms_b, fail=None, verify_ok=(True, True)):
    log = []

    def prepare(name, first):
        log.append(("prepare", name, first))
        return {"name": name}

    def capture(h, name):
        log.append(("capture", name))
        if fail == name:
            raise bench.CaptureBroken("injected")

        def a():
            return ms_a * 1e-3

        def b():
            return ms_b * 1e-3
        return a if name == "after_backward" else b

    def verify(h, run, name):
        ok = verify_ok[0 if name == "after_backward" else 1]
        return {"ok": ok, "weights_rel_l2": 1e-4 if ok else 3.0}, ok
    clock = _Clock()
    after = []
    recs, chosen, failure = bench.measure_exchange_schedules(["after_backward", "bucketed_overlap"], prepare, capture, clock, 20, 6,
                                                             verify, lambda rec: after.append(rec["handle"]["name"]))
    return recs, chosen, failure, clock.calls, log, after


def test_a_failed_capture_of_the_second_schedule_keeps_the_first_schedules_graph_measurement():
    recs, chosen, failure, calls, log, after = _schedules(31.0, 30.0, fail="bucketed_overlap")
    assert failure is not None and failure[0] == "bucketed_overlap"
    assert chosen == "after_backward"                            # a finished, graph-replayed, FULL region
    assert recs["after_backward"]["dt"] == pytest.approx(20 * 31e-3) and recs["after_backward"]["check"]["ok"]
    assert "bucketed_overlap" not in recs
    assert calls == [("a", 20)]                                  # the full region of A ran BEFORE B was even prepared
    assert log.index(("capture", "bucketed_overlap")) > log.index(("capture", "after_backward"))
    assert after == ["after_backward"]


def test_a_failed_capture_of_the_first_schedule_reports_nothing_graphed():
    recs, chosen, failure, calls, _, _ = _schedules(31.0, 30.0, fail="after_backward")
    assert failure[0] == "after_backward" and chosen is None and recs == {} and calls == []


def test_the_faster_schedule_runs_its_own_full_region_and_wins():
    recs, chosen, failure, calls, _, after = _schedules(31.0, 30.0)
    assert failure is None and chosen == "bucketed_overlap"
    assert calls == [("a", 20), ("b", 6), ("b", 20)]
    assert recs["bucketed_overlap"]["ab_ms"] == pytest.approx(30.0) and recs["after_backward"]["ab_ms"] == pytest.approx(31.0)
    assert after == ["after_backward", "bucketed_overlap"]


def test_a_slower_second_schedule_gets_no_full_region():
    recs, chosen, failure, calls, _, _ = _schedules(30.0, 31.5)
    assert failure is None and chosen == "after_backward" and calls == [("a", 20), ("b", 6)]
    assert recs["bucketed_overlap"]["dt"] is None and recs["bucketed_overlap"]["ab_ms"] == pytest.approx(31.5)


def test_a_replay_that_does_not_reproduce_the_eager_step_is_never_the_timed_value():
    recs, chosen, _, calls, _, _ = _schedules(31.0, 30.0, verify_ok=(False, True))
    assert chosen == "bucketed_overlap" and recs["after_backward"]["dt"] is None and ("a", 20) not in calls
    recs, chosen, _, calls, _, _ = _schedules(31.0, 30.0, verify_ok=(True, False))
    assert chosen == "after_backward" and recs["bucketed_overlap"]["dt"] is None
    recs, chosen, _, _, _, _ = _schedules(31.0, 30.0, verify_ok=(False, False))
    assert chosen is None and all(v["dt"] is None for v in recs.values())


def test_counter_passes_are_tied_to_the_library(tmp_path, monkeypatch):
    me = bench.library_identity()
    assert len(me["lib_sha256"]) == 64 and len(me["src_sha256"]) == 64 and me["sources"] >= 20
    assert bench.counters_current({"lib_sha256": me["lib_sha256"], "src_sha256": "x"}) == "library sha256"
    assert bench.counters_current({"lib_sha256": "x", "src_sha256": me["src_sha256"]}) == "source sha256"
    assert bench.counters_current({"lib_sha256": "x", "src_sha256": "y"}) is None
    assert bench.counters_current(None) is None                   # a file without the record (an older round's) is stale

    class A:
        arch, batch = "resnet50_mrlal", 256
    assert bench.measure_exchange_schedules is bench_ranks.measure_exchange_schedules and bench.pmc_traffic is bench_report.pmc_traffic
    monkeypatch.setattr(bench_report, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench_report, "library_identity", lambda: me)
    os.makedirs(tmp_path / "profiles")
    path = tmp_path / "profiles" / f"{bench.ROUND}_pmc_traffic_resnet50_mrlal_b256.json"
    rec = {"light_apply_bwd": {"hbm_bytes_per_launch": 1.1e9}}
    path.write_text(json.dumps(dict(rec, _meta={"lib_sha256": me["lib_sha256"]})))
    assert bench.pmc_traffic(A, "mrla_light_apply_bwd")[0] == 1100000000
    path.write_text(json.dumps(dict(rec, _meta={"lib_sha256": "0" * 64, "src_sha256": "1" * 64})))
    assert bench.pmc_traffic(A, "mrla_light_apply_bwd") == (None, os.path.join("profiles", path.name), "stale")
    path.write_text(json.dumps(rec))
    assert bench.pmc_traffic(A, "mrla_light_apply_bwd")[2] == "stale"
    path.unlink()
    assert bench.pmc_traffic(A, "mrla_light_apply_bwd") == (None, None, None)


def _record(monkeypatch, argv, **more):
    """What core.Run hands report() for a single-process run whose 4 timed steps of 256 images took 0.2 s (no GPU needed)."""
    import torch
    from benchkit import common
    from mrla_amd import functional as Fm
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    args = common.parse()
    R = dict(args=args, rank=0, world=1, seen=1, dist_on=False, dp="none", layout="channels_last", x=torch.zeros(1, 3, 224, 224),
             net=None, exchange=None, schedule=None, ab_ms=None, legs=True, replay=None, rank_ms=None, what="fwd+bwd+SGD",
             ddp_first=None, full=bool(args.full), dt=0.2, dt_eager=None, dt_events=None, timer=Fm.KernelTimer(), use_graph=True,
             launch="one HIP graph per step", in_sync=None, finite=True)
    R.update(more)
    return R


def test_a_plain_run_prints_the_headline_and_measures_nothing_beside_it(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` is run several times per change: its line carries the contract keys and
    `ms_per_step`, and none of the legs that take runs of their own -- those wait for --full (report() would have to touch a
    GPU, the host cores or a child process to produce them: none is there for it here)."""
    from benchkit import baselines
    for leg in ("forward_only", "eager_rocm", "eager_rocm_detection", "cpu_baseline", "run_drop_path_0", "run_other_configs",
                "run_detection_backbone"):
        monkeypatch.setattr(baselines, leg, lambda *a, **k: pytest.fail("a leg beside the headline ran in a plain run"))
    rec = json.loads(bench_report.report(_record(monkeypatch, ["--gpus", "1", "--steps", "4", "--warmup", "1"]), emit=False))
    assert rec["metric"] == "images/sec fwd+bwd resnet50_mrlal b=256" and rec["unit"] == "images/sec"
    assert rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["steps"] == 4 and rec["warmup"] == 1
    assert rec["ms_per_step"] == 50.0 and rec["value"] == 256 * 4 / 0.2
    for key in ("roofline", "mrla_kernels", "eager_launch_ms_per_step", "eager_launch_images_per_sec", "forward_only", "eager_rocm",
                "cpu_baseline", "other_configs", "detection_backbone"):
        assert key not in rec, key
    assert "drop_path_0" not in rec["config"]


def test_full_moves_nothing_out_of_the_line(monkeypatch):
    """--full: every leg beside the headline is asked for, in the line under the key it always had."""
    from benchkit import baselines
    for leg in ("forward_only", "eager_rocm", "cpu_baseline", "run_drop_path_0", "run_other_configs", "run_detection_backbone"):
        monkeypatch.setattr(baselines, leg, lambda *a, _leg=leg, **k: {"leg": _leg, "fwd_images_per_sec": 1.0})
    monkeypatch.setattr("torch.cuda.empty_cache", lambda: None)
    rec = json.loads(bench_report.report(_record(monkeypatch, ["--steps", "4", "--full"], dt_eager=0.25, dt_events=0.3), emit=False))
    assert rec["ms_per_step"] == 50.0 and rec["eager_launch_ms_per_step"] == 62.5 and "roofline" in rec and "mrla_kernels" in rec
    assert rec["forward_only"]["leg"] == "forward_only" and rec["eager_rocm"]["leg"] == "eager_rocm"
    assert rec["cpu_baseline"]["leg"] == "cpu_baseline" and rec["config"]["drop_path_0"]["leg"] == "run_drop_path_0"
    assert rec["other_configs"]["leg"] == "run_other_configs" and rec["detection_backbone"]["leg"] == "run_detection_backbone"
    # ... and the child processes of those legs are --full runs themselves (they report roofline / eager_rocm to their parent)
    seen = {}

    def no_child(cmd, **k):
        seen["cmd"] = cmd
        raise baselines.subprocess.TimeoutExpired(cmd, 0)
    monkeypatch.setattr(baselines.subprocess, "run", no_child)
    assert baselines._child(["--arch", "resnet101_mrlab"])[0] is None
    assert "--full" in seen["cmd"] and "--no-baselines" in seen["cmd"]


def test_dumped_outputs_are_the_same_positions_every_time(tmp_path):
    """--dump-outputs: vectors above SAMPLE elements are written as one fixed, seeded, sorted sample; small ones whole; float32."""
    import numpy as np
    import torch
    from benchkit import outputs
    big = [torch.arange(outputs.SAMPLE, dtype=torch.float32), torch.arange(outputs.SAMPLE, 3 * outputs.SAMPLE, dtype=torch.float32)]
    a, b = outputs._flat_sample(big), outputs._flat_sample([t.clone() for t in big])
    assert a.dtype == np.float32 and a.shape == (outputs.SAMPLE,) and np.array_equal(a, b) and np.all(np.diff(a) >= 0)
    assert a.max() > 2 * outputs.SAMPLE                              # (drawn from the whole vector, not from its head)
    small = outputs._flat_sample([torch.ones(3, 2), torch.zeros(4)])
    assert small.tolist() == [1.0] * 6 + [0.0] * 4
    outputs.write(str(tmp_path / "d"), {"loss": np.float32([1.5]), "weights": small})
    assert np.load(tmp_path / "d" / "loss.npy").tolist() == [1.5] and np.load(tmp_path / "d" / "weights.npy").dtype == np.float32
    assert 3 * 4 * outputs.SAMPLE <= 64 << 20


def test_committed_miopen_records_go_into_a_private_directory(monkeypatch):
    """bench.py hands MIOpen a COPY of benchkit/miopen_db/ (it writes into its user databases), never the committed files; an
    environment that names its own directory, or an outside launcher's ranks, keep what they have."""
    from benchkit import common
    committed = sorted(f for f in os.listdir(common.MIOPEN_DB) if f.endswith(".txt"))
    assert len(committed) == 2 and all(f.startswith("gfx950") for f in committed)
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    d = common.use_committed_miopen_tuning()
    try:
        assert os.environ["MIOPEN_USER_DB_PATH"] == d and os.path.realpath(d) != os.path.realpath(common.MIOPEN_DB)
        assert sorted(os.listdir(d)) == committed
        for f in committed:
            assert open(os.path.join(d, f), "rb").read() == open(os.path.join(common.MIOPEN_DB, f), "rb").read()
        assert common.use_committed_miopen_tuning() is None and os.environ["MIOPEN_USER_DB_PATH"] == d
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
        monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert common.use_committed_miopen_tuning() is None and "MIOPEN_USER_DB_PATH" not in os.environ
