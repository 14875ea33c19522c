"""Build nanorepeat_amd/libnanorepeat_amd.so (HIP kernels + C ABI) in-tree for gfx950.

hipcc cross-compiles without a GPU.  The kernel file is split into parts
(-DNRA_PART=1..43) that compile in parallel; the shared library carries only gfx950 code.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
LIB = os.path.join(HERE, "libnanorepeat_amd.so")
OBJ = os.path.join(HERE, "csrc", "build")

# the kernel files and the parts (-DNRA_PART) each is compiled in
KERNELS = (("nra_kernels.hip", (1, 2, 3, 4)),
           ("nra_sweep.hip", (5, 6, 11, 12, 13, 14, 15, 16, 18, 19, 25, 26)),
           ("nra_joint.hip", (7, 8, 10, 17, 20, 21, 22, 23)),
           ("nra_trace.hip", (9,)),
           ("nra_screen.hip", (27,)),
           ("nra_structure.hip", (28,)),
           ("nra_motif.hip", (29,)),
           ("nra_extend.hip", (30,)),
           ("nra_mixture.hip", (31,)),
           ("nra_consensus.hip", (32,)),
           ("nra_split.hip", (33,)),
           ("nra_segment.hip", (34,)),
           ("nra_period.hip", (35,)),
           ("nra_screen_motifs.hip", (36,)),
           ("nra_bootstrap.hip", (37,)),
           ("nra_flank.hip", (38,)),
           ("nra_censored.hip", (39,)),
           ("nra_methyl.hip", (40,)),
           ("nra_scan.hip", (41,)),
           ("nra_sketch.hip", (42,)),
           ("nra_place.hip", (43,)))
HOSTS = ("nra_host.cpp", "nra_plan1d.cpp", "nra_plan2d.cpp", "nra_screen_host.cpp", "nra_structure_host.cpp", "nra_motif_host.cpp", "nra_extend_host.cpp",
         "nra_mixture_host.cpp", "nra_consensus_host.cpp", "nra_split_host.cpp", "nra_segment_host.cpp",
         "nra_period_host.cpp", "nra_bootstrap_host.cpp", "nra_flank_host.cpp", "nra_censored_host.cpp", "nra_methyl_host.cpp",
         "nra_scan_host.cpp", "nra_sketch_host.cpp", "nra_place_host.cpp")
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
SOURCES = [k for k, _ in KERNELS] + list(HOSTS) + HEADERS
ARCH = "gfx950"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(INCLUDE, "nanorepeat_amd.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, jobs=None, verbose=False):
    """Compile and link the shared library; returns its path."""
    if not force and not _stale():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    common = [hipcc, f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-I", INCLUDE, "-I", CSRC,
              "-Wno-unused-command-line-argument"]
    cmds = []
    objs = []
    for kernel, parts in KERNELS:
        for part in parts:
            o = os.path.join(OBJ, f"{kernel[:-len('.hip')]}_p{part}.o")
            objs.append(o)
            cmds.append(common + [f"-DNRA_PART={part}", "-c", os.path.join(CSRC, kernel), "-o", o])
    for host in HOSTS:
        o = os.path.join(OBJ, host[:-len(".cpp")] + ".o")
        objs.append(o)
        cmds.append(common + ["-pthread", "-c", os.path.join(CSRC, host), "-o", o])

    # an object is rebuilt when its source, a header next to it or the public header is newer
    headers = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(INCLUDE, "nanorepeat_amd.h")]

    def fresh(cmd):
        obj, src = cmd[-1], cmd[-3]
        if force or not os.path.exists(obj):
            return False
        t = os.path.getmtime(obj)
        return all(os.path.getmtime(d) <= t for d in [src] + headers)

    cmds = [c for c in cmds if not fresh(c)]

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)

    jobs = jobs or max(1, min(len(cmds), max(1, (os.cpu_count() or 2) - 1)))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(run, cmds))
    run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-pthread", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
