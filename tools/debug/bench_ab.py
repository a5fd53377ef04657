"""A/B of two builds of libgeoadv.so on the headline (MEASUREMENT TOOLING; needs the GPU):

    python tools/debug/bench_ab.py --parent PARENT.so --new NEW.so [--arm NAME=OTHER.so ...] [--runs 5] [--out ab.txt]

For K = 500 and K = 20: `bench.py --gpus 1 --steps K --warmup 20` (plain run: headline ms_per_step) and, in a process of its
own, bench.py's small_batch_sweep at the same K (B = 16 / 8 / 4), parent and new (and every further --arm) alternating, --runs process runs each; the
library file is swapped between runs (and the new one is left in place at the end).  --dump-outputs of the first 500-step run of
each build is compared byte for byte.  VERDICT lines: the new build's median against the parent's own min-max range of the
session.  Every child runs under a time limit; the first failure ends the session (nothing else is started on the GPU).
"""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB = os.path.join(ROOT, "geometric_adv_amd", "lib", "libgeoadv.so")


def sweep_child(steps):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from geometric_adv_amd import dist as gdist, weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    weights = W.synthetic_weights(bench.N, seed=7)
    ae = PointNetAE(weights, bench.N, device=dev)
    out = bench.small_batch_sweep(dev, weights, ae, 20, steps, gdist, "nccl", bench.Watchdog(0, 120.0))
    print(json.dumps({str(k): v["ms_per_step"] for k, v in out.items()}))


def last_json(text):
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError("no JSON line in: %s" % text[-500:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new")
    ap.add_argument("--name", default="new")
    ap.add_argument("--arm", action="append", default=[], metavar="NAME=PATH", help="a further build, measured like --new")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep-child", type=int, default=None)
    a = ap.parse_args()
    if a.sweep_child is not None:
        return sweep_child(a.sweep_child)
    libs = {"parent": a.parent, a.name: a.new, **dict(arm.split("=", 1) for arm in a.arm)}
    lines, rows, dumps = [], {}, {}
    tmp = tempfile.mkdtemp(prefix="bench_ab_")

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def child(cmd):
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            say("FAILED rc %d: %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-2000:]))
            finish(1)
        return last_json(r.stdout)

    def finish(rc):
        shutil.copyfile(a.new, LIB)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(rc)

    for k in (500, 20):
        for i in range(a.runs):
            for build, path in libs.items():
                shutil.copyfile(path, LIB)
                t0 = time.time()
                cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(k), "--warmup", "20"]
                if k == 500 and i == 0:
                    dumps[build] = os.path.join(tmp, build)
                    cmd += ["--dump-outputs", dumps[build]]
                head = child(cmd)
                sweep = child([sys.executable, os.path.abspath(__file__), "--sweep-child", str(k)])
                row = {"ms": head["ms_per_step"], "b16": sweep["16"], "b8": sweep["8"], "b4": sweep["4"]}
                rows.setdefault((k, build), []).append(row)
                say("%s %d ms_per_step %.6f B16 %.6f B8 %.6f B4 %.6f (%d s)" % (build, k, row["ms"], row["b16"], row["b8"], row["b4"], time.time() - t0))
    same = True
    for arm in [b for b in libs if b != "parent"]:
        for k in (500, 20):
            for key in ("ms", "b16", "b8", "b4"):
                p = [r[key] for r in rows[(k, "parent")]]
                n = [r[key] for r in rows[(k, arm)]]
                verdict = ("median BELOW the parent's minimum" if median(n) < min(p) else
                           "median within the parent's range" if median(n) <= max(p) else "median SLOWER than the parent's range")
                say("VERDICT K=%d %s parent min %.6f median %.6f max %.6f | %s min %.6f median %.6f max %.6f | %s %s" % (
                    k, key, min(p), median(p), max(p), arm, min(n), median(n), max(n), arm, verdict))
        names = sorted(os.listdir(dumps["parent"]))
        eq = names == sorted(os.listdir(dumps[arm])) and all(
            filecmp.cmp(os.path.join(dumps["parent"], f), os.path.join(dumps[arm], f), shallow=False) for f in names)
        same = same and eq
        say("DUMP %s: --dump-outputs of the first 500-step run, %d files %s: %s" % (arm, len(names), names, "byte-identical" if eq else "DIFFERENT"))
    finish(0 if same else 1)


if __name__ == "__main__":
    main()
