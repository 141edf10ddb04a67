"""CPU: bench.py's command line.  A plain `bench.py --gpus 1 --steps N --warmup W` switches every measurement beside the headline off;
`--full` switches them back on, each still droppable by its own --no-... option."""
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _off(args):
    import bench
    return {name for name in bench.EXTRAS if getattr(args, "no_" + name)}


def test_plain_run_switches_every_extra_off():
    import bench
    args = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not args.full and _off(args) == set(bench.EXTRAS)
    assert (args.gpus, args.steps, args.warmup, args.batch, args.seq, args.layers, args.dtype) == (1, 5, 2, 4, 2048, 32, "bf16")
    assert _off(bench.parse_args([])) == set(bench.EXTRAS)
    assert _off(bench.parse_args(["--dump-outputs", "somewhere"])) == set(bench.EXTRAS)


def test_full_switches_every_extra_on_and_keeps_the_run_the_same():
    import bench
    plain = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    full = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2", "--full"])
    assert full.full and _off(full) == set()
    skip = {"full"} | {"no_" + name for name in bench.EXTRAS}
    assert {k: v for k, v in vars(plain).items() if k not in skip} == {k: v for k, v in vars(full).items() if k not in skip}
    # every extra has its own switch, and main() reads no other no_... attribute
    assert {k for k in vars(full) if k.startswith("no_")} >= {"no_" + name for name in bench.EXTRAS}
    assert _off(bench.parse_args(["--full", "--no-dropin", "--no-cpu-baseline"])) == {"dropin", "cpu_baseline"}
    for name in bench.EXTRAS:
        assert _off(bench.parse_args(["--full", "--no-" + name.replace("_", "-")])) == {name}


def test_full_is_accepted_by_the_dry_run():
    bench = os.path.join(ROOT, "bench.py")
    lines = []
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, bench, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dry-run"] + extra, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
    a, b = lines
    assert set(a) == set(b)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert a[key] == b[key], key
