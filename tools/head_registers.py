"""Kernel metadata of the 32 fused-head instantiations (csrc/head_inst_*.hip: fp16 / bf16 x anchor padding TNA = 1..4 x single / group launch x NA = 1 / NA = 3) of two
source trees side by side, and of the class-filter twins (template parameter FILT) a tree has, each against the parent's kernel of the same form -- the recipe of profiles/best_class_head_registers.txt and profiles/class_filter_head_registers.txt: hipcc -O3 --offload-arch=gfx950 -S, device
code only, so it runs on a machine without a GPU.

    python tools/head_registers.py PARENT_TREE [THIS_TREE] [--jobs 8] [--keep DIR]
prints one line per kernel: VGPR / AGPR / SGPR / scratch bytes / occupancy (waves per SIMD) of either tree.  kern 1 = NA 1, 2 = NA 3; 1f / 2f = their class-filter twins."""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-x", "hip"]
FIELDS = ("NumVGPRsForWavesPerEU", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy")


def metadata(tree, unit, out_dir):
    asm = os.path.join(out_dir, unit.replace(".hip", ".s"))
    if not os.path.exists(asm):   # (--keep: a listing from an earlier call is reused)
        subprocess.run(["hipcc", *FLAGS, os.path.join(tree, "yolort_amd", "csrc", unit), "-o", asm + ".tmp"], check=True, capture_output=True)
        os.replace(asm + ".tmp", asm)
    kernels, name = {}, None
    for line in open(asm):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r";\s*(\w+):\s*(\d+)\s*$", line)
        if m and name and m.group(1) in FIELDS:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
    rows = {}
    for k, v in kernels.items():
        na = int(re.findall(r"Li(\d+)E", k)[2])   # <dtype, TNA, NA[, FILT]>
        rows[("1" if na == 1 else "2") + ("f" if "Lb1E" in k else "")] = "/".join(str(v[f]) for f in FIELDS)
    return rows, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this", nargs="?", default=ROOT)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", default=None, help="directory that keeps the assembly listings (DIR/parent, DIR/this) instead of a temporary one")
    args = ap.parse_args()
    units = sorted(f for f in os.listdir(os.path.join(args.this, "yolort_amd", "csrc")) if f.startswith("head_inst_") and f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(args.jobs) as ex:
        a, b = os.path.join(args.keep or tmp, "parent"), os.path.join(args.keep or tmp, "this")
        os.makedirs(a, exist_ok=True), os.makedirs(b, exist_ok=True)
        old = list(ex.map(lambda u: metadata(args.parent, u, a), units))
        new = list(ex.map(lambda u: metadata(args.this, u, b), units))
    print("kernel metadata of the fused-head instantiations (gfx950, -O3), parent commit -> this commit")
    print(f"{'translation unit':<28} kern  {'parent v/a/s/scratch/occ':<22} {'this v/a/s/scratch/occ':<22} same")
    n, same_all, worse = 0, True, []
    for u, (o, ok), (w, wk) in zip(units, old, new):
        for kern in sorted(w):
            ref = o[kern.rstrip("f")]   # a class-filter twin is held against the parent's kernel of the same form
            same = ref == w[kern]
            if not kern.endswith("f"):
                same_all &= same
                n += 1
            print(f"{u.replace('.hip', '.s'):<28} {kern:<5} {ref:<22} {w[kern]:<22} {'yes' if same else 'NO'}")
            po, pw = [int(x) for x in ref.split("/")], [int(x) for x in w[kern].split("/")]
            if pw[4] < po[4] or (po[3] == 0 and pw[3] > 0):
                worse.append((u, kern))
    print(f"kernels: {n} all figures equal: {same_all}; occupancy dropped or scratch appeared in: {worse if worse else 'none'}")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
