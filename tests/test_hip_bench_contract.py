"""GPU: the driver's contract with bench.py — ONE JSON line with the metric of BASELINE.json, the roofline and cpu_baseline
objects, a frame verified against the oracle — for the plain 1-GPU invocation and for the launch the driver uses for N > 1
(`python -m torch.distributed.run ... bench.py --gpus N`, here with one rank: RCCL communicator, streamed frame gather, barriers,
max-over-ranks timing)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
SMALL = ["--steps", "6", "--warmup", "2", "--roofline-steps", "3"]


def _bench(args, launched):
    """The full record (--details FILE), after checking the printed line: exactly one, short, and the record's summary."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable]
    if launched:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", "29561"]
    with tempfile.TemporaryDirectory() as tmp:
        details = os.path.join(tmp, "details.json")
        r = subprocess.run(cmd + [os.path.join(ROOT, "bench.py")] + args + ["--details", details], capture_output=True, text=True, timeout=900,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]  # exactly one JSON line
        assert len(lines[0]) < 4096, len(lines[0])  # whole in any tail of the output
        line = json.loads(lines[0])
        d = json.load(open(details))
    assert line["details"] == details
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "wsum_mean", "hit_fraction"):
        assert line[k] == d[k], k
    assert line["kernel_ms"] == d["roofline"]["kernel_ms"] and line["roofline"]["frac"] == d["roofline"]["frac"]
    assert ("verify_ok" in line) == ("verify" in d) and line.get("verify_ok") == d.get("verify", {}).get("ok")
    return d


def _check_line(d, steps, scene="surface"):
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"].startswith("rendered rays/sec at 512") and base["metric"].startswith("rendered rays/sec at 512")
    assert d["unit"] == "rays/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["vs_baseline"] is None and d["value"] > 1e6
    assert abs(d["value"] - 512 * 512 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]  # whole-job rays / wall time of the K steps
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["scene"] == scene
    r = d["roofline"]
    assert r["unit"] == "GB/s" and r["bound"] in ("hbm", "l2") and "traffic" in r
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] <= 1.0  # never achieved > peak under its own label
    # the headline pair is self-consistent: `frac` belongs to the TIMED launch — the algorithmic bytes of the decode
    # steps it executed / its own HIP-event time — so what the line implies for the wall-clock step cannot exceed the HBM peak
    assert abs(r["algorithmic_bytes_executed"] - r["algorithmic_bytes_per_launch"] * r["decode_steps_executed_frac"]) < 1.0
    assert r["algorithmic_bytes_per_launch"] == 512 * 512 * (96 * 1536 + 172) and 0 < r["decode_steps_executed_frac"] <= 1
    hbm_timed = r["algorithmic_bytes_executed"] / (r["kernel_ms"] * 1e-3) / 1e9
    if r["bound"] == "hbm":
        assert r["peak"] == 8000.0 and abs(r["achieved"] - hbm_timed) < 1e-6 * hbm_timed
        assert r["algorithmic_bytes_executed"] / (d["ms_per_step"] * 1e-3) <= 8.0e12 and r["kernel_ms"] <= d["ms_per_step"] * 1.02
        assert abs(r["frac"] * r["peak"] * 1e9 * r["kernel_ms"] * 1e-3 - r["algorithmic_bytes_executed"]) < 1e-6 * r["algorithmic_bytes_executed"]
    else:  # the yardstick exceeded the HBM peak: relabelled to the L2-level gather fraction, algorithmic figure kept beside it
        assert r["peak"] == 34500.0 and abs(r["hbm_algorithmic_equiv_frac"] - hbm_timed / 8000.0) < 1e-6 and hbm_timed > 8000.0
    # ... and the SURVEY 8(d) contract figure (every algorithmic sample decoded) sits beside it under its own name
    full = r["algorithmic_bytes_per_launch"] / (r["kernel_ms_no_early_out"] * 1e-3) / 1e9
    assert abs(r["frac_full_work"] - full / 8000.0) < 1e-9 and abs(r["achieved_full_work"] - full) < 1e-6 * full
    assert r["kernel_ms_no_early_out"] >= r["kernel_ms"] * 0.98 and "frac_timed" not in r
    assert r["compulsory_bytes_per_launch"] == 3 * 32 * 256 * 256 * 4 + 512 * 512 * 172
    if r["traffic"]:
        assert abs(r["hbm_measured_frac"] - r["traffic"] / (r["kernel_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9 and r["hbm_measured_frac"] < 1.0
        assert abs(r["traffic_over_compulsory"] - r["traffic"] / r["compulsory_bytes_per_launch"]) < 1e-9
        assert r["compulsory_bytes_incl_draws"] == r["compulsory_bytes_per_launch"] + 512 * 512 * 96 * 4
        assert abs(r["traffic_over_compulsory_incl_draws"] - r["traffic"] / r["compulsory_bytes_incl_draws"]) < 1e-9
    else:
        assert r["hbm_measured_frac"] is None and r["traffic_over_compulsory"] is None
    w = d["config"]["workload"]
    assert "checkpoint ecrutileE_eclustrousC_n120" in w and "absent" in w and "UNPINNED against skimage / kornia" in w
    ph = r["physical"]["l2_gather"]
    assert 0 < ph["frac_no_early_out"] <= 1.0 and 0 < ph["frac_timed"] <= 1.0
    v = d["verify"]
    assert v["ok"] is True and v["exact"]["ok"] and v["tolerance"]["ok"]
    # non-vacuous: the verified scene has a real surface, the exact mode is bit-identical to the oracle, PSNR vs the reference itself
    assert v["exact"]["wsum_mean"] > 0.2 and all(v["exact"][k]["bit_exact_vs_oracle"] for k in ("feat", "depth", "wsum", "xyz"))
    for m in ("exact", "tolerance"):
        rb = v[m]["reference_block"]
        assert rb["ok"] and (isinstance(rb["psnr_vs_reference_db"], str) or rb["psnr_vs_reference_db"] > 80.0)
        assert rb["rays_beyond_tolerance_unexplained"] == 0
    # SURVEY 8(d) "inds and sort permutation: exact-match count = 100 % or reported mismatch count with cause", at BASELINE scale, against
    # the REFERENCE's own indices (not the oracle's): the counts of tests/test_oracle_golden.py::test_bench_block_index_parity_with_cause
    ip = v["exact"]["reference_block"]["index_parity"]
    assert (ip["inds_mismatch"], ip["perm_mismatch"], ip["mask_flips"], ip["rays_beyond_tolerance"]) == (1, 4, 1, 1) and ip["inds_total"] == 196608
    assert ip["all_explained"] and ip["dump_launch_equals_production_launch"]
    assert ip["inds_mismatch_detail"][0]["u_ulps_to_reference_cdf_edge"] <= 1.0 and ip["mask_flip_detail"][0]["cause"] == "cull threshold"
    ip96 = v["eval_faithful_exact"]["reference_block"]["index_parity"]
    assert (ip96["inds_mismatch"], ip96["perm_mismatch"], ip96["mask_flips"], ip96["rays_beyond_tolerance"]) == (0, 12, 0, 0) and ip96["all_explained"]
    top = d["index_parity"]
    assert top["48+48"]["inds_mismatch"] == 1 and top["48+48"]["inds_total"] == 196608 and top["96+96"]["inds_mismatch"] == 0 and top["96+96"]["all_explained"]


PIPELINE_KEYS = ("backbone_ms", "sr_ms", "g_f_view_ms", "c2_ms", "c5_512_ms")


def test_bench_default_invocation_prints_the_contract_line():
    d = _bench(SMALL, launched=False)
    _check_line(d, 6)
    assert d["dtype"] == "f32" and d["config"]["final_pass"] == "exact"  # the exact contract is what is timed, on the surface scene
    assert d["hit_fraction"] > 0.3 and d["wsum_mean"] > 0.2
    rows = {(r["scene"], r["mode"]) for r in d["results"]}
    assert rows == {(s, m) for s in ("canonical", "surface") for m in ("exact", "tolerance")}
    assert all(r["kernel_ms"] > 0 and r["kernel_ms_no_early_out"] > 0 and 0 < r["decode_steps_executed_frac"] <= 1 for r in d["results"])
    assert len(d["eval_faithful"]["rows"]) == 4 and all(r["Sc"] == 96 and r["Sf"] == 96 for r in d["eval_faithful"]["rows"])
    # the SURVEY 8(d) scene (an empty volume) and the eval-faithful 96+96 sit at the top level, next to the surface-scene headline
    rc = next(r for r in d["results"] if r["scene"] == "canonical" and r["mode"] == "exact")
    rs = next(r for r in d["results"] if r["scene"] == "surface" and r["mode"] == "exact")
    rf = next(r for r in d["eval_faithful"]["rows"] if r["scene"] == "surface" and r["mode"] == "exact")
    assert d["value_canonical"] == rc["rays_per_s"] and d["ms_per_step_canonical"] == rc["ms_per_step"] and d["kernel_ms_canonical"] == rc["kernel_ms"]
    assert d["value_surface"] == rs["rays_per_s"] and d["ms_per_step_surface"] == rs["ms_per_step"]
    assert d["value_surface_96p96"] == rf["rays_per_s"] and d["ms_per_step_surface_96p96"] == rf["ms_per_step"]
    assert rs["hit_fraction"] > 0.3 and rc["hit_fraction"] == 0.0 and "EMPTY volume" in d["scene_note"]
    assert abs(d["value"] - d["value_surface"]) < 0.25 * d["value"]  # the headline IS the surface scene (re-timed in the table)
    assert d["sustained"]["seconds"] >= 2.0 and d["sustained"]["sustained_ms_per_step"] > 0
    assert d["device_rng"]["ms_per_step"] > 0 and d["device_rng"]["kernel_ms"] > 0  # the opt-in in-kernel draws, beside the contract step
    rec = d["roofline"]["recorded"]  # PMC numbers are builder-recorded and say so; absent capture -> nulls, never stale numbers
    assert "source" in rec and (rec["bounds"] is None or rec["bounds"].get("valu_active_frac", 0) <= 1.0)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and c["unit"] == "rays/s" and c["sample"]
    assert "per_rank" not in d
    # the callers either side of the renderer, under the same clock
    p = d["pipeline"]
    assert "error" not in p, p
    assert all(p[k] > 0 for k in PIPELINE_KEYS) and p["seconds"] < 60
    assert p["backbone"]["GFLOP"] > 90 and p["superresolution"]["GFLOP"] > 150 and p["g_f_view"]["ms_with_paste"] > p["g_f_view_ms"] * 0.9
    assert p["c2"]["batch"] == 4 and p["c5_512"]["points"] == 512 ** 3 and p["c5_512"]["faces"] > 0
    assert "source" in p["mfma_busy_recorded"]
    # round 6: the convolution path under the driver's clock with its own roofline object — GPU time of a pass
    # replayed from a hipGraph, the live launch count of that capture, the fraction of the two-term MFMA peak
    for k, max_launches in (("backbone", 60), ("superresolution", 20)):
        r = p[k]
        assert r["kernel_us"] > 0 and r["kernel_us"] * 1e-3 <= r["ms"] * 1.05 and 0 < r["frac_of_two_term_peak"] < 1
        assert r["launches"] is None or 0 < r["launches"] <= max_launches, (k, r["launches"])
        assert r["roofline"]["bound"] == "mfma" and abs(r["roofline"]["frac"] - r["frac_of_two_term_peak"]) < 1e-9
    assert p["g_f_view"]["replayed"] is True
    # item 8: the tolerance-mode headline beside the exact one (same scene, same K); ADVICE r05: both timing passes of a table row
    assert d["value_tolerance"] > d["value_surface"] * 0.95 and d["ms_per_step_tolerance"] > 0
    assert all(len(r["ms_per_step_passes"]) == 2 and min(r["ms_per_step_passes"]) == r["ms_per_step"] for r in d["results"])


def test_bench_canonical_scene_is_still_a_switch():
    d = _bench(SMALL + ["--scene", "canonical", "--no-cpu-baseline", "--no-table", "--no-pipeline"], launched=False)
    _check_line(d, 6, scene="canonical")
    assert d["hit_fraction"] == 0.0 and d["roofline"]["decode_steps_executed_frac"] < 0.6 and "EMPTY volume" in d["config"]["workload"]


def test_bench_under_torch_distributed_run_streams_the_frames():
    d = _bench(SMALL + ["--no-cpu-baseline", "--no-pipeline"], launched=True)
    _check_line(d, 6)
    assert len(d["per_rank"]["ms_per_step_render"]) == 1 and len(d["per_rank"]["gather_ms"]) == 1
    assert "slices sent while the next frames render" in d["config"]["workload"]
    assert d["n_ranks_seen"] == 1
    g = d["gather"]
    assert g["mode"].startswith("streamed") and g["bytes_into_rank0"] == 0 and g["frame_bytes"] == 512 * 512 * 16 and g["exposed_ms_max"] >= 0
    assert g["backend"].startswith("nccl")
    e = _bench(SMALL + ["--no-cpu-baseline", "--no-table", "--no-pipeline", "--gather", "end", "--fast"], launched=True)
    _check_line(e, 6)
    assert "pipeline" not in d and "pipeline" not in e
    assert e["dtype"].startswith("f32 (final-pass MLP operands as two-term f16") and "ONE gather" in e["config"]["workload"]
    assert "results" not in e and "value_surface" not in e and e["gather"]["mode"].startswith("end")


def test_bench_views_per_step_renders_v_views_per_launch():
    """`--views-per-step V`: V views of the subject in ONE renderer launch (planes shared by the batch, per-view depth clamp) — the
    whole-job value counts V x 512^2 rays per step, the roofline's per-launch byte counts scale with V, the verification still passes."""
    d = _bench(["--steps", "4", "--warmup", "1", "--roofline-steps", "2", "--views-per-step", "3", "--no-table", "--no-pipeline", "--no-cpu-baseline"],
               launched=False)
    assert d["config"]["views_per_step"] == 3 and d["config"]["rays_per_step_per_gpu"] == 3 * 512 * 512
    assert abs(d["value"] - 3 * 512 * 512 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    r = d["roofline"]
    assert r["algorithmic_bytes_per_launch"] == 3 * 512 * 512 * (96 * 1536 + 172) and 0 < r["frac"] <= 1.0
    assert d["verify"]["ok"] is True and "3 views per GPU per step in ONE launch" in d["config"]["workload"]


def _dump_run(tmp, run, extra=()):
    import numpy as np
    args = ["--steps", "3", "--warmup", "1", "--roofline-steps", "0", "--no-table", "--no-pipeline", "--no-cpu-baseline", "--no-verify", *extra]
    out = os.path.join(tmp, run)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", out], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert sorted(os.listdir(out)) == ["depth.npy", "feat.npy", "wsum.npy", "xyz.npy"]
    return line, {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}


def test_bench_dump_outputs_are_the_last_steps_and_repeat():
    """`--dump-outputs DIR`: the arrays the timed step returned in its last step (feat, depth, wsum, xyz), float32, <= 16 MB; two runs
    with the same arguments render the same inputs, so they dump the same bytes.  A 512^2 frame (38 MB) is dumped as one seeded sample
    of rays taken from every array; a 256^2 frame whole, in the shapes the caller receives."""
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        (la, a), (_, b) = _dump_run(tmp, "a"), _dump_run(tmp, "b")
        ls, small = _dump_run(tmp, "small", ["--res", "256"])
    assert la["steps"] == 3 and sum(x.nbytes for x in a.values()) <= 16 << 20
    n = a["feat"].shape[0]
    assert 0.25 * 512 * 512 < n < 512 * 512
    for k, c in (("feat", 32), ("depth", 1), ("wsum", 1), ("xyz", 3)):
        assert a[k].dtype == np.float32 and a[k].shape == (n, c) and np.array_equal(a[k], b[k]), k
    assert abs(float(a["wsum"].astype(np.float64).mean()) - la["wsum_mean"]) < 0.02 and a["wsum"].max() > 0.5  # a sample of the frame
    R = 256 * 256
    for k, c in (("feat", 32), ("depth", 1), ("wsum", 1), ("xyz", 3)):
        assert small[k].dtype == np.float32 and small[k].shape == (1, R, c), k
    assert abs(float(small["wsum"].astype(np.float64).mean()) - ls["wsum_mean"]) < 1e-5  # the line's wsum_mean is the last step's


def test_bench_side_tables_take_a_fixed_number_of_steps():
    """`--steps K` sets the timed region; the side tables and the device_rng row take min(K, --table-steps) steps, so a run's wall
    time is the K timed steps plus a fixed cost, whatever K is."""
    d = _bench(["--steps", "40", "--warmup", "2", "--roofline-steps", "2", "--no-pipeline", "--no-cpu-baseline", "--no-verify"], launched=False)
    assert d["steps"] == 40
    assert all(r["steps"] == 20 for r in d["results"]) and all(r["steps"] == 10 for r in d["eval_faithful"]["rows"])
    assert d["device_rng"]["steps"] == 20
