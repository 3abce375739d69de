"""Static census of one kernel's gfx950 ISA: registers, scratch and the opcode counts of its loops.

Compiles ONE .hip file of thermo_nerf_amd/csrc with the Makefile's flags to assembly (hipcc --cuda-device-only -S; no GPU
needed), finds the kernels whose demangled name contains the given text, and prints for each its VGPR / AGPR / SGPR counts,
scratch bytes, LDS bytes, and for every loop (a label and the last branch back to it) the opcode histogram of its body.  A loop's
body includes the loops nested in it.

usage: python tools/isa_census.py thermo_nerf_amd/csrc/tn_render_mfma.hip 'main_mfma_rays_kernel<true, false>' [--extra=-DX=1]
           [--min-insts N]   only loops of at least N instructions (default 200)
           [--top N]         the N most frequent opcodes per loop (default: all)
           [--json]          one JSON object instead of text

As a module: census(path, name, extra=()) -> [{"name", "vgpr", "agpr", "sgpr", "scratch", "lds", "loops": [{"label", "depth",
"insts", "ops": {opcode: count}}]}]; sample_loop(kernel) picks the shortest loop that holds matrix instructions: for the field
kernels that is the per-sample loop (the tile loop around it adds the 32 MFMAs of the per-tile SH bias).
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thermo_nerf_amd", "csrc")


def hipcc() -> str | None:
    return shutil.which(os.environ.get("HIPCC", "hipcc")) or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def makefile_flags() -> list[str]:
    """The FLAGS line of csrc/Makefile with its make variables resolved (no -fPIC needed for -S, but harmless)."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


def assemble(path: str, extra=()) -> str:
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "census.s")
        cmd = [cc, *makefile_flags(), *extra, "--cuda-device-only", "-S", f"-I{os.path.dirname(os.path.abspath(path))}",
               path, "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.PIPE)
        return open(out).read()


def demangle(symbols: list[str]) -> dict[str, str]:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    for cand in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        if filt is None and os.path.exists(cand):
            filt = cand
    if filt is None:
        return {s: s for s in symbols}
    res = subprocess.run([filt], input="\n".join(symbols), capture_output=True, text=True, check=True)
    return dict(zip(symbols, res.stdout.splitlines()))


_INST = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def loops_of(body: list[str]) -> list[dict]:
    labels = {}
    for n, line in enumerate(body):
        m = _LABEL.match(line)
        if m:
            labels[m.group(1)] = n
    back = {}  # label -> last line that branches back to it
    for n, line in enumerate(body):
        m = _BRANCH.match(line)
        if m and m.group(1) in labels and labels[m.group(1)] < n:
            back[m.group(1)] = n
    spans = sorted((labels[lab], end, lab) for lab, end in back.items())
    loops = []
    for a, b, lab in spans:
        ops = collections.Counter()
        for line in body[a:b + 1]:
            m = _INST.match(line)
            if m:
                ops[m.group(1)] += 1
        depth = 1 + sum(1 for a2, b2, _ in spans if a2 <= a and b <= b2 and (a2, b2) != (a, b))
        loops.append({"label": lab, "depth": depth, "insts": sum(ops.values()), "ops": dict(ops.most_common())})
    return loops


def census(path: str, name: str, extra=()) -> list[dict]:
    text = assemble(path, extra)
    lines = text.splitlines()
    starts = [(n, m.group(1)) for n, line in enumerate(lines) if (m := re.match(r"^(_Z\w+):", line))]
    names = demangle([s for _, s in starts])
    want = name.replace(" ", "")
    out = []
    for n, sym in starts:
        if want not in names[sym].replace(" ", ""):
            continue
        end = next(k for k in range(n, len(lines)) if lines[k].strip().startswith("s_endpgm"))
        desc = "\n".join(lines[end:end + 400])

        def field(key, desc=desc):
            m = re.search(r"\." + key + r"\s+(\d+)", desc)
            return int(m.group(1)) if m else None

        m_acc = re.search(r"; AccumOffset:\s*(\d+)", desc)
        m_arch = re.search(r"; NumVgprs:\s*(\d+)", desc)
        m_agpr = re.search(r"; NumAgprs:\s*(\d+)", desc)
        m_sgpr = re.search(r"; NumSgprs:\s*(\d+)", desc)
        m_scr = re.search(r"; ScratchSize:\s*(\d+)", desc)
        out.append({
            "name": names[sym], "symbol": sym,
            "vgpr": int(m_arch.group(1)) if m_arch else None,
            "agpr": int(m_agpr.group(1)) if m_agpr else None,
            "vgpr_total": field("amdhsa_next_free_vgpr"),
            "accum_offset": int(m_acc.group(1)) if m_acc else None,
            "sgpr": int(m_sgpr.group(1)) if m_sgpr else None,
            "scratch": int(m_scr.group(1)) if m_scr else field("amdhsa_private_segment_fixed_size"),
            "lds": field("amdhsa_group_segment_fixed_size"),
            "loops": loops_of(lines[n:end + 1]),
        })
    return out


def sample_loop(kernel: dict) -> dict:
    with_mfma = [lp for lp in kernel["loops"] if any(op.startswith("v_mfma") for op in lp["ops"])]
    return min(with_mfma, key=lambda lp: lp["insts"])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source")
    ap.add_argument("kernel", help="text the demangled kernel name must contain (blanks ignored)")
    ap.add_argument("--extra", action="append", default=[], help="one more compiler flag, e.g. --extra=-DTN_FIELD_STAMPS=1")
    ap.add_argument("--min-insts", type=int, default=200)
    ap.add_argument("--top", type=int, default=0)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    found = census(args.source, args.kernel, args.extra)
    if not found:
        print("no kernel matches", args.kernel, file=sys.stderr)
        return 1
    if args.json:
        print(json.dumps(found))
        return 0
    for k in found:
        print(f"{k['name']}\n  vgpr {k['vgpr']}  agpr {k['agpr']}  allocated {k['vgpr_total']}  sgpr {k['sgpr']}  "
              f"scratch {k['scratch']} B  static lds {k['lds']} B")
        for lp in k["loops"]:
            if lp["insts"] < args.min_insts:
                continue
            print(f"  loop {lp['label']} depth {lp['depth']}: {lp['insts']} instructions")
            ops = list(lp["ops"].items())
            for op, c in ops[:args.top] if args.top else ops:
                print(f"    {c:6d}  {op}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
