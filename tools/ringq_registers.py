"""Registers of every k_sweep_ringq instantiation, with and without the saturation events around the step loop.

The events ("The saturation exit") run where the whole wave state is live; what keeps them from costing
registers -- 8-byte pieces, loads serialised through an empty asm, an occupancy hint the kernel can meet -- depends on the
compiler, so this script holds it to account on the CPU: it cross-compiles the parts of nra_sweep.hip that instantiate
k_sweep_ringq for gfx950 to assembly, as they are and with -DNRA_SAT_EXIT=0, reads the kernels' metadata (VGPRs, waves per
SIMD, scratch bytes) from the compiler's own summary comments, prints one row per instantiation and exits with status 1
if any instantiation has fewer waves per SIMD with the events than without.

    python tools/ringq_registers.py [--jobs N] [--markdown]        (ten minutes of four hipcc processes)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanorepeat_amd import build as B      # noqa: E402

PARTS = (25, 26)                            # full-wave and half-wave k_sweep_ringq
NAME = re.compile(r"^_Z13k_sweep_ringqILi(\d+)ELb([01])ELb([01])ELb([01])EE\w*:")
FIELDS = (("vgpr", re.compile(r"; NumVgprs: (\d+)")), ("scratch", re.compile(r"; ScratchSize: (\d+)")),
          ("waves", re.compile(r"; Occupancy: (\d+)")))


def compile_part(part, out, extra):
    cmd = [B._hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-fPIC", "-std=c++17", "-I", B.INCLUDE, "-I", B.CSRC,
           "-Wno-unused-command-line-argument", "-Wno-pass-failed", f"-DNRA_PART={part}", "-S", "--cuda-device-only",
           os.path.join(B.CSRC, "nra_sweep.hip"), "-o", out] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr[-2000:])
    return out


def kernels(path):
    """{(R, has_n, half, taint): {vgpr, scratch, waves}} from the summary comments behind each kernel."""
    out, cur = {}, None
    for line in open(path):
        m = NAME.match(line)
        if m:
            cur = tuple(int(x) for x in m.groups())
            out[cur] = {}
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = pat.search(line)
            if m:
                out[cur][key] = int(m.group(1))
                if key == "waves":
                    cur = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(p, os.path.join(tmp, f"{tag}_{p}.s"), extra) for p in PARTS
                for tag, extra in (("with", []), ("without", ["-DNRA_SAT_EXIT=0"]))]
        with ThreadPoolExecutor(max_workers=args.jobs) as ex:
            list(ex.map(lambda j: compile_part(*j), jobs))
        with_, without = {}, {}
        for p in PARTS:
            with_.update(kernels(os.path.join(tmp, f"with_{p}.s")))
            without.update(kernels(os.path.join(tmp, f"without_{p}.s")))
    lost = []
    sep = " | " if args.markdown else "  "
    print(sep.join(["R", "HAS_N", "HALF", "TAINT", "VGPRs", "waves", "scratch"]))
    for k in sorted(with_, key=lambda k: (k[2], k[0], k[1], k[3])):
        a, b = without[k], with_[k]
        print(sep.join([str(k[0]), str(k[1]), str(k[2]), str(k[3]), f"{a['vgpr']} -> {b['vgpr']}", f"{a['waves']} -> {b['waves']}",
                        f"{a['scratch']} -> {b['scratch']}"]))
        if b["waves"] < a["waves"]:
            lost.append(k)
    print(f"{len(with_)} instantiations; fewer waves with the events: {lost or 'none'}")
    return 1 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
