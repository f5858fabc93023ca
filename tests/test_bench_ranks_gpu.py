"""bench.py's N-rank path end to end on one GPU: `bench.py --gpus 2` through
torch.distributed.run with every rank on device 0 and gloo in place of RCCL
(SHADOWTOPO_BENCH_ONE_GPU with --full, which RCCL cannot do: it refuses two ranks on one device).  The
launcher, the source sharding, the packed (dense) row codec, the exchange, the barriers and
the rank-0 report all run as on N GPUs; each rank then checks the matrix the exchange
assembled against the whole matrix its own engine computes, bit for bit (bench.rehearsal_check).
A small C2 (scale 0.1, dense: packed rows) and C4 (scale 0.02, sparse: 16-bit hop
counts) keep it to seconds; the full-size C2 and C4 rehearsals at 2 and 4
ranks are recorded in profiles/r06z2_rank_rehearsal/."""
import json
import os
import signal
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("config,scale,ranks,mode", [("C2", 0.1, 2, "packed"), ("C2", 0.1, 3, "packed"),
                                                     ("C4", 0.02, 2, "hops16")])
def test_bench_rank_rehearsal_assembles_the_exact_matrix(config, scale, ranks, mode):
    env = dict(os.environ, SHADOWTOPO_BENCH_ONE_GPU="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "2", "--warmup", "1",
           "--config", config, "--scale", str(scale), "--full", "--no-north-star", "--no-fresh", "--no-host-rate"]
    # its own process group: a hung run is ended with every rank the launcher started
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         start_new_session=True)
    try:
        out, err = p.communicate(timeout=110)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        pytest.fail("the rank rehearsal did not finish in 110 s")
    assert p.returncode == 0, err[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert lines, out[-2000:]
    out = json.loads(lines[-1])
    assert out["n_gpus"] == ranks and "rehearsal" in out
    chk = out["rehearsal_check"]
    assert chk["lat_equal"] and chk["rel_equal"] and chk["hops_equal"], chk
    assert chk["ranks_equal"] == [True] * ranks, chk
    assert out["exchange"]["mode"] == mode, out["exchange"]
    assert sum(out["sharding"]["per_rank_rows"]) == out["config"]["attached"], out["sharding"]


@pytest.mark.gpu
def test_plain_bench_times_the_steps_only_and_dumps_their_rows(tmp_path):
    """A plain `bench.py --gpus 1` run (no --full) reports the headline figures of exactly
    --steps timed steps and none of the side measurements; --dump-outputs writes the rows the
    last timed step left on the device as float64 arrays, equal bit for bit to the rows an
    engine of this process computes for the same seeded workload (small C2, scale 0.1)."""
    import numpy as np

    import bench
    from shadow_amd import engine as E
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "C2", "--scale", "0.1", "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "source-paths/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["steps"] == 3 and out["warmup"] == 1
    rows = out["config"]["sources_per_gpu"]
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(rows / out["ms_per_step"] * 1e3, rel=1e-9)
    for key in ("cpu_baseline", "north_star", "shim_host_matrix"):
        assert out[key] is None, key
    for key in ("matrix_build_host_ms", "matrix_build_fresh_ms"):
        assert out["config"][key] is None, key
    assert out["engine"]["host_buffers_ms"] is None and "probe_rows" not in out["exchange"]

    g, _per, _desc = bench.build_workload("C2", 1, 0.1)
    eng = E.Engine.from_synth(g, device=0)
    try:
        eng.set_attached(g.attached)
        lat, rel, hops, _kind = eng.compute_rows()
    finally:
        eng.close()
    got = {n: np.load(dump / f"{n}.npy") for n in ("latency", "reliability", "hops")}
    assert sorted(os.listdir(dump)) == ["hops.npy", "latency.npy", "reliability.npy"]
    assert all(a.dtype == np.float64 and a.shape == (rows, len(g.attached)) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BYTES
    assert np.array_equal(got["latency"].view(np.uint64), lat.view(np.uint64))
    assert np.array_equal(got["reliability"].view(np.uint64), rel.view(np.uint64))
    assert np.array_equal(got["hops"], hops.view(np.int32).astype(np.float64))
