"""CPU suite: the bench line kept under profiles/ carries every field of the bench.py contract (metric, value ...,
roofline, cpu_baseline), and bench.py's option surface is the one the driver uses.  GPU part: a plain run measures the
headline alone and --dump-outputs writes what its last timed step computed."""
import json
import os
import re

import pytest

from conftest import ROOT


def latest_line():
    names = sorted((f for f in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"r\d+_bench_v\d+\.json", f)),
                   key=lambda f: [int(x) for x in re.findall(r"\d+", f)])
    with open(os.path.join(ROOT, "profiles", names[-1])) as f:
        return names[-1], json.load(f)


def test_bench_line_has_the_contract_fields():
    name, d = latest_line()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, (name, k)
    assert d["unit"] == "modexp/s" and d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c.get("bit_exact_vs_gpu") is True
    # the value is elements / time of the timed steps
    assert abs(d["value"] - d["config"]["elements_per_gpu"] * d["n_gpus"] / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6


def test_bench_options():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert f'"{opt}"' in src
    # the product legs never import the oracle: only the two cpu_baseline blocks do
    body = src.split("def main() -> None:")[1]
    head, tail = body.split("if rank == 0 and not args.no_cpu:")
    assert "oracle" not in head.replace('"oracle", "libvmnoracle.so"', "")


def _run_bench(args, env_extra, timeout=300):
    import subprocess
    import sys
    env = dict(os.environ, OMP_NUM_THREADS="1", **env_extra)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout, env=env)


def test_bench_starts_its_own_ranks_when_typed_without_a_launcher(entry):
    """`python3 bench.py --gpus N` (the way the driver types the N = 1 command) must not exit with "use a launcher": the
    parent spawns `torch.distributed.run` as a child before touching the GPU, relays rank 0's line and its exit code."""
    pr = _run_bench(["--gpus", "3", "--steps", "2", "--warmup", "0", "--scaling", "strong"], {"VMN_BENCH_LAUNCH_ONLY": "1"})
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, pr.stdout.decode()
    d = json.loads(lines[0])
    assert d == {"launch_only": True, "n_gpus": 3, "scaling": "strong", "steps": 2}
    # without a GPU the ranks refuse to run (no CPU fallback) and the parent hands their failure on
    pr = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {})
    err = pr.stderr.decode()
    assert pr.returncode != 0 and "no GPU visible" in err and "must be launched" not in err
    assert "rehearsal" in err                          # fewer GPUs than ranks: the parent says what kind of run this is


def test_launched_rank_count_must_match_gpus():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "self_launch(args)" in src and "WORLD_SIZE" in src
    assert '"--scaling"' in src and "strong" in src


def test_plain_run_leaves_the_legs_and_baselines_to_full():
    """Everything after the headline (modexp_by_shape, the mix / decryption legs, the CPU baselines) runs under --full only."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src.split("def main() -> None:")[1]
    head, gated = body.split("    if args.full:\n")
    gated = gated.split("\n    if rank == 0:\n")[0]
    for call in ('guarded("modexp_by_shape"', 'guarded("mix_prove"', 'guarded("decrypt_2048"', 'guarded("mix_ccpos_3072"',
                 'guarded("mix_ec_p256"', "orc.exp_array_bytes(", "cpu_mix_prove(", "cpu_decrypt("):
        assert call not in head and call in gated, call
    for line in gated.splitlines():
        assert not line.strip() or line.startswith("        "), line


@pytest.mark.gpu
def test_plain_run_dumps_the_output_of_its_last_step(entry, tmp_path):
    """`bench.py --steps 2 --dump-outputs DIR`: one line with the headline fields and none of --full's, steps as asked,
    and DIR/modexp_out.npy = the seeded sample of out[] = x^e mod p, equal to the GMP oracle on the same inputs."""
    import numpy as np
    bench = _load_bench()
    n = bench.DUMP_SAMPLE + 3000                      # more than the sample: the seeded subset is what is written
    pr = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--elements", str(n), "--dump-outputs", str(tmp_path)], {})
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, pr.stdout.decode()
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - n / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    for k in ("modexp_by_shape", "mix_prove", "decrypt_2048", "mix_ccpos_3072", "mix_ec_p256", "cpu_baseline"):
        assert k not in d, k
    got = np.load(os.path.join(tmp_path, "modexp_out.npy"))
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_SAMPLE, 256)
    idx = bench.dump_index(n)
    xb, eb = bench.make_inputs(n, 20260000, 256)
    x = np.frombuffer(xb, dtype=np.uint8).reshape(n, 256)[idx]
    e = np.frombuffer(eb, dtype=np.uint8).reshape(n, 256)[idx]
    from oracle.cbind import Oracle
    p, q, g = bench.load_sub(entry, "stdgroups").modp_group(2048)
    orc = Oracle(p, q, 256)
    orc.set_threads(min(len(os.sched_getaffinity(0)), 16))
    want = np.frombuffer(orc.exp_array_bytes(x.tobytes(), e.tobytes(), len(idx), 256), dtype=np.uint8).reshape(len(idx), 256)
    assert np.array_equal(got, want.astype(np.float32))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_dump", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m
