#!/usr/bin/env python3
"""Register / scratch table of the sweep kernels from their code objects (no GPU needed): compiles vimure_amd/csrc/sweep_sl.hip
for every K to assembly and reads the kernel descriptors' metadata.  Writes a markdown table (stdout or --out).

  python tools/kernel_resources.py [--out profiles/r03_kernel_resources.md] [--k 2 3 ...]

With --unit NAME: the same table (and the static LDS) of every kernel of vimure_amd/csrc/NAME.hip instead.

  python tools/kernel_resources.py --unit centrality [--notes FILE] [--out profiles/centrality_kernel_resources.md]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vimure_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def asm_for(k, tmp):
    out = os.path.join(tmp, f"sl_k{k}.s")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    f"-DVMR_K={k}", "--offload-device-only", "-S", "-o", out, os.path.join(CSRC, "sweep_sl.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def rows(k, text):
    out = []
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        name, blk = m.group(1), m.group(2)
        t = re.search(r"k_sweep_sl(_b)?ILi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])(?:ELb([01]))?(?:ELb([01]))?E", name)
        if not t:
            continue
        lock = t.group(1) is not None
        # (k_sweep_sl<.., STORE, DET, LPD>, k_sweep_sl_b<.., STORE, LPD>)
        lpd = (t.group(8) if not lock else t.group(7)) == "1"
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        upd, elbo, full, store, det = t.group(3) == "1", t.group(4) == "1", t.group(5) == "1", t.group(6) == "1", t.group(7) == "1" and not lock
        variant = ("update+ELBO" if elbo else "update") if upd else ("ELBO only" if elbo else "statistics only")
        if not store:
            variant += ", rho not written"
        if det:
            variant += ", deterministic"
        if lpd:
            variant += ", log-prior difference"
        if lock:
            variant += " (lockstep)"
        vg = g("vgpr_count")
        alloc = (vg + 7) // 8 * 8
        out.append((k, variant, "all ones" if full else "any", vg, min(8, 512 // max(alloc, 1)), g("sgpr_count"), g("vgpr_spill_count"),
                    g("sgpr_spill_count"), g("private_segment_fixed_size")))
    return out


def unit_table(unit):
    """Every kernel of vimure_amd/csrc/<unit>.hip: registers, static LDS and scratch from the code object's metadata."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "--offload-device-only", "-S", "-o", out, os.path.join(CSRC, unit + ".hip")], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    rows_ = []
    meta = text[text.index("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - (?=\.)", meta)[1:]:   # one entry per kernel, its keys in alphabetical order
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        short = re.sub(r"^void ", "", re.sub(r"\(anonymous namespace\)::", "", short)).split("(")[0]
        vg, ag = g("vgpr_count"), g("agpr_count")
        alloc = (vg + ag + 7) // 8 * 8
        rows_.append((short, f"{vg} (+{ag})", min(8, 512 // max(alloc, 1)), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"),
                      g("group_segment_fixed_size"), g("private_segment_fixed_size")))
    lines = [f"# The kernels of {unit}.hip: registers, LDS and scratch (code-object metadata, gfx950)", "",
             f"From `hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude -Ivimure_amd/csrc --offload-device-only -S vimure_amd/csrc/{unit}.hip`"
             " (`python tools/kernel_resources.py --unit " + unit + "`).", "",
             "| kernel | VGPRs (+AGPRs) | waves/SIMD by VGPRs | SGPRs | VGPR spills | SGPR spills | static LDS B | scratch B/lane |",
             "|---|---|---|---|---|---|---|---|"]
    lines += ["| " + " | ".join(str(v) for v in r) + " |" for r in sorted(rows_)]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--k", type=int, nargs="*", default=[2, 3, 4, 5, 6, 7, 8])
    ap.add_argument("--unit", help="a translation unit of vimure_amd/csrc other than the sweep (centrality, connectivity, ..): every kernel of it")
    ap.add_argument("--notes", help="with --unit: a text file appended below the table")
    a = ap.parse_args()
    if a.unit:
        text = unit_table(a.unit)
        if a.notes:
            text += "\n" + open(a.notes).read()
        if a.out:
            open(a.out, "w").write(text)
        sys.stdout.write(text)
        return
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(len(a.k), os.cpu_count() or 1)) as ex:
        texts = list(ex.map(lambda k: asm_for(k, tmp), a.k))
    table = [r for k, t in zip(a.k, texts) for r in sorted(rows(k, t), key=lambda r: (r[1], r[2]))]
    lines = ["# k_sweep_sl<K, UPDATE, ELBO, ALLFULL, STORE, DET, LPD> / k_sweep_sl_b<K, UPDATE, ELBO, ALLFULL, STORE, LPD>: registers and scratch per variant (code-object metadata, gfx950)", "",
             "SGPR spills go to VGPR lanes (v_writelane), not to memory; `VGPR spills` and `scratch` are what costs.", "",
             "| K | variant | mask rows | VGPRs | waves/SIMD by VGPRs | SGPRs | VGPR spills | SGPR spills | scratch B/lane |", "|---|---|---|---|---|---|---|---|---|"]
    lines += ["| " + " | ".join(str(v) for v in r) + " |" for r in table]
    text = "\n".join(lines) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
