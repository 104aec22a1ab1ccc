"""bench.py launches its own ranks when it is not under torchrun: `python bench.py --gpus 2` must spawn two processes
(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), run the sharded entry point with one all-gather per global batch and print
ONE JSON line with n_gpus 2.  Exercised on the CPU with the script's stub engine over gloo (--stub)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--steps", "2", "--warmup", "1"] + extra,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("[Gloo]")]    # (gloo's own connect banner)
    assert len(lines) == 1, r.stdout                      # stdout carries the ONE JSON line (rank 0 only)
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    d = _run(["--gpus", "2"])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 8               # 4 images per rank


def test_bench_sharded_global_batch_smaller_than_world_times_micro():
    d = _run(["--gpus", "2", "--global-batch", "3"])      # ragged shards (2 + 1): still one line, strong scaling
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["global_batch"] == 3


def test_bench_single_rank_stub():
    d = _run([])
    assert d["n_gpus"] == 1 and d["value"] > 0


def test_bench_cites_the_final_collection_of_the_newest_round(tmp_path, monkeypatch):
    """`roofline.traffic` comes from profiles/rNN_traffic.json of the newest round — the round's FINAL collection, not an earlier one
    of the same round (rNNa_ / rNNe_ sort after rNN_ alphabetically and were picked up once)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    prof = tmp_path / "profiles"
    prof.mkdir()
    for name, val in (("r05_traffic.json", 1.0), ("r06_traffic.json", 2.0), ("r06a_traffic.json", 3.0), ("r06e_traffic.json", 4.0)):
        (prof / name).write_text(json.dumps({"head": name, "conv3": {"hbm_bytes_per_launch": val}}))
    (prof / "r06_traffic_inflight_plans.json").write_text(json.dumps({"conv3": {"hbm_bytes_per_launch": 5.0}}))
    (prof / "r06e_traffic_inflight_plans.json").write_text(json.dumps({"conv3": {"hbm_bytes_per_launch": 6.0}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.measured_traffic() == (2.0, "r06_traffic.json @ r06_traffic.json")
    assert bench.measured_traffic_inflight_plans()[0] == 5.0


def test_bench_dump_outputs_writes_the_last_timed_step_reproducibly(tmp_path):
    """--dump-outputs DIR writes the frames the timed path returned for its last step as DIR/frames.npy (float32, [G, 3, H, W]);
    the same arguments give the same arrays, and --steps K makes the K-th timed step the one written"""
    import numpy as np
    outs = {}
    for tag, extra in (("a", []), ("b", []), ("k3", ["--steps", "3"])):
        d = _run(["--dump-outputs", str(tmp_path / tag)] + extra)
        assert d["steps"] == (3 if tag == "k3" else 2)
        assert sorted(os.listdir(tmp_path / tag)) == ["frames.npy"]
        outs[tag] = np.load(tmp_path / tag / "frames.npy")
    assert outs["a"].dtype == np.float32 and outs["a"].shape == (4, 3, 4, 4)
    assert np.array_equal(outs["a"], outs["b"])
    assert not np.array_equal(outs["a"], outs["k3"])          # step 3's batch and seed, not step 2's


def test_bench_dump_outputs_samples_an_output_over_the_budget(tmp_path, monkeypatch):
    """an output larger than the 64 MB budget is written as a fixed, seeded sample of its elements plus their flat indices"""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    t = torch.arange(2 * 3 * 20 * 20, dtype=torch.float32).reshape(2, 3, 20, 20)
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), {"frames": t})
        assert sorted(os.listdir(tmp_path / tag)) == ["frames_sample.npy", "frames_sample_index.npy"]
    v, i = np.load(tmp_path / "a" / "frames_sample.npy"), np.load(tmp_path / "a" / "frames_sample_index.npy")
    assert v.dtype == np.float32 and i.dtype == np.float64 and v.shape == i.shape == (100,)
    assert np.array_equal(v, t.numpy().reshape(-1)[i.astype(np.int64)])
    assert np.array_equal(v, np.load(tmp_path / "b" / "frames_sample.npy"))


def test_bench_threaded_weight_fill_equals_fill_module():
    """bench.py builds its engine with the synthetic weights drawn on several threads and moved to the device one tensor at a
    time (fill_weights_): every value is synth.fill_module_'s, bit for bit (a reduced-width UNet, on the host)"""
    import importlib.util
    import torch
    import udifftext_amd  # noqa: F401  (puts the sgm mirror on sys.path)
    from sgm.modules.diffusionmodules.openaimodel import UnifiedUNetModel
    from sgm.util import skip_param_init
    from udifftext_amd import synth
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def unet():
        with skip_param_init():
            return UnifiedUNetModel(in_channels=9, ctrl_channels=0, model_channels=64, out_channels=4, num_res_blocks=1,
                                    attention_resolutions=[1, 2], channel_mult=[1, 2], num_head_channels=64,
                                    use_linear_in_transformer=True, transformer_depth=1, t_context_dim=128,
                                    save_attn_type=["t_attn"])
    want, got = unet(), unet()
    synth.fill_module_(want)
    bench.fill_weights_(got, torch.device("cpu"), threads=4)
    sw, sg = want.state_dict(), got.state_dict()
    assert list(sw) == list(sg) and len(sw) > 100
    assert all(sw[k].dtype == sg[k].dtype and torch.equal(sw[k], sg[k]) for k in sw)
