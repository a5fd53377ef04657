"""Static instruction counts of the encoder forward kernels (MEASUREMENT TOOLING; needs hipcc, no GPU):

    python tools/encoder_isa_counts.py [--label new] [--source geometric_adv_amd/csrc/encoder_x3.hip]

compiles the source to gfx950 assembly with the Makefile's flags and prints, per kernel whose name matches --kernels, the VALU
(v_* other than MFMAs), MFMA and s_nop instruction counts, the register counts, spills and the scratch size the compiler
reports.  The kernels are straight-line, so the static count is the count per wave.  profiles/r12_encoder_isa_counts.txt holds
its output for the commit before the mix-instruction split and for the tree.
"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize"]


def counts(asm, pattern):
    rows = []
    name, c = None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, c = m.group(1), {"valu": 0, "mfma": 0, "s_nop": 0, "lshl_add_u64": 0, "mix": 0}
            continue
        if name is None:
            continue
        t = line.strip()
        op = t.split()[0] if t else ""
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["lshl_add_u64"] += op == "v_lshl_add_u64"
            c["mix"] += op.startswith("v_fma_mix")
        elif op == "s_nop":
            c["s_nop"] += 1
        for key, tag in (("vgprs", "NumVgprs"), ("agprs", "NumAgprs"), ("sgprs", "TotalNumSgprs"), ("scratch", "ScratchSize")):
            m = re.match(r"^;\s*%s:\s*(\d+)" % tag, t)
            if m:
                c[key] = int(m.group(1))
        if t.startswith("; Occupancy"):
            if re.search(pattern, name):
                rows.append((name, c))
            name = None
    # the spill counts stand in the code object's metadata only
    spills = {}
    for block in re.split(r"\n\s*- \.agpr_count:", asm)[1:]:
        m = re.search(r"\.name:\s*(_Z\S+)", block)
        if m:
            spills[m.group(1)] = tuple(int(re.search(r"\.%s_spill_count:\s*(\d+)" % k, block).group(1)) for k in ("vgpr", "sgpr"))
    for name, c in rows:
        c["vgpr_spill"], c["sgpr_spill"] = spills.get(name, (None, None))
    return rows


def demangled(name):
    try:
        return subprocess.run(["/opt/rocm/llvm/bin/llvm-cxxfilt", name], capture_output=True, text=True, check=True).stdout.strip().split("(")[0]
    except (OSError, subprocess.CalledProcessError):
        return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(ROOT, "geometric_adv_amd", "csrc", "encoder_x3.hip"))
    ap.add_argument("--kernels", default=r"encoder_fwd3s?_kernelILi2ELb1E")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--asm", default=None, help="count this assembly file instead of compiling --source")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            subprocess.run([a.hipcc] + FLAGS + ["-S", "--offload-device-only", a.source, "-o", out], check=True, stderr=subprocess.DEVNULL)
            asm = open(out).read()
    for name, c in counts(asm, a.kernels):
        print("%s %s: VALU %d (v_lshl_add_u64 %d, v_fma_mix* %d) MFMA %d s_nop %d | VGPRs %s AGPRs %s SGPRs %s | VGPR spills %s SGPR spills %s scratch %s bytes" % (
            a.label, demangled(name), c["valu"], c["lshl_add_u64"], c["mix"], c["mfma"], c["s_nop"], c.get("vgprs"), c.get("agprs"),
            c.get("sgprs"), c.get("vgpr_spill"), c.get("sgpr_spill"), c.get("scratch")))


if __name__ == "__main__":
    main()
