"""Phase stamps of main_mfma_rays_kernel: where the two waves of a SIMD pair are, sample by sample.

Builds an instrumented copy of the library (tn_render_mfma.hip with -DTN_FIELD_STAMPS=1, linked with the objects `make` left in
csrc/build/; the shipped library is not touched), renders bench.py's frame with it in this process and reads the stamp buffer back:
for 16 workgroups, waves 0 and 4 (one SIMD pair), every sample of the wave's second tile, s_memtime at 16 phase boundaries.

usage:  python tools/field_stamps.py --build-only            (no GPU needed: writes thermo_nerf_amd/libthermonerf_hip_stamps.so)
        python tools/field_stamps.py [--out profiles/micro/field_phase_stamps_S192.txt] [--extra=-DX=1]
Ticks are s_memtime's own unit; compare phases with each other, not with the unstamped kernel (the stamps drain the scalar
memory counter at every boundary).
"""
from __future__ import annotations

import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "thermo_nerf_amd", "csrc")
LIB = os.path.join(ROOT, "thermo_nerf_amd", "libthermonerf_hip_stamps.so")
BLOCKS, SAMPLES, SLOTS = 16, 192, 16
PHASES = ["position + taps 0", "gather wait 0", "blend 0 + taps 1", "gather wait 1", "blend 1 + taps 2", "gather wait 2",
          "blend 2 + taps 3", "gather wait 3", "blend 3", "base layers", "colour head", "colour output layer", "thermal head",
          "thermal sigmoid + output", "compositing", "stamp store + loop"]
MLP = range(9, 14)  # phases between slot 9 (hash done) and slot 14


def build(extra):
    import isa_census

    objs = [os.path.join(CSRC, "build", f) for f in sorted(os.listdir(os.path.join(CSRC, "build")))
            if f.endswith(".o") and f != "tn_render_mfma.o"]
    assert objs, "run make in thermo_nerf_amd/csrc first"
    obj = os.path.join(CSRC, "build", "stamps_tn_render_mfma.o_")
    cc = isa_census.hipcc()
    subprocess.run([cc, *isa_census.makefile_flags(), "-DTN_FIELD_STAMPS=1", *extra, "-c", os.path.join(CSRC, "tn_render_mfma.hip"),
                    "-o", obj], check=True)
    subprocess.run([cc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, obj, "-o", LIB], check=True)
    os.remove(obj)


def analyse(buf, out):
    import numpy as np

    t = np.asarray(buf, dtype=np.int64).reshape(BLOCKS, 2, SAMPLES, SLOTS)
    used = [b for b in range(BLOCKS) if t[b, :, :, 0].all()]
    print(f"# workgroups with both partners stamped: {len(used)} of {BLOCKS}", file=out)
    dur = np.zeros((2, SLOTS))
    overlap = np.zeros((2, SLOTS, SLOTS + 1))  # [wave][own phase][partner phase | partner outside its stamped tile]
    for b in used:
        tl = []
        for w in range(2):
            x = t[b, w].copy()
            flat = x.reshape(-1)
            flat[:] = flat[0] + np.cumsum(np.concatenate([[0], (np.diff(flat) & 0xFFFFFFFF)]))  # undo the 32-bit wrap
            tl.append(flat)
        for w in range(2):
            own, oth = tl[w], tl[1 - w]
            for k in range(len(own) - 1):
                p = k % SLOTS
                a0, a1 = own[k], own[k + 1]
                dur[w, p] += a1 - a0
                i0 = np.searchsorted(oth, a0, "right") - 1
                c = a0
                while c < a1:
                    if i0 < 0:
                        nxt = min(a1, oth[0]); q = SLOTS
                    elif i0 >= len(oth) - 1:
                        nxt = a1; q = SLOTS
                    else:
                        nxt = min(a1, oth[i0 + 1]); q = i0 % SLOTS
                    overlap[w, p, q] += nxt - c
                    c = nxt
                    i0 += 1
    n = len(used) * SAMPLES
    print("# mean ticks per sample and phase; beside it, the share of that time the PARTNER spent in: its hash phase (slots 0-9),\n"
          "# of which waiting for gathers; its MLP block (matrix + vector); compositing/loop; outside its stamped tile", file=out)
    print(f"{'phase':28s} {'wave':>4s} {'ticks':>8s} {'%sample':>8s} | {'p.hash':>7s} {'p.gwait':>7s} {'p.mlp':>7s} {'p.comp':>7s} {'p.out':>7s}", file=out)
    for p in range(SLOTS):
        for w in range(2):
            o = overlap[w, p]
            tot = max(o.sum(), 1)
            hashp = o[0:9].sum() / tot; gw = o[[1, 3, 5, 7]].sum() / tot; mlp = o[9:14].sum() / tot
            comp = o[14:16].sum() / tot; outside = o[16] / tot
            print(f"{PHASES[p]:28s} {4 * w:4d} {dur[w, p] / n:8.1f} {100 * dur[w, p] / dur[w].sum():8.2f} | {100 * hashp:7.1f} "
                  f"{100 * gw:7.1f} {100 * mlp:7.1f} {100 * comp:7.1f} {100 * outside:7.1f}", file=out)
    for w in range(2):
        print(f"# wave {4 * w}: ticks per sample {dur[w].sum() / n:.1f}; hash phase {dur[w, 0:9].sum() / n:.1f}, MLP block "
              f"{dur[w, 9:14].sum() / n:.1f}", file=out)
    # how the partners line up along the march: entry of wave 4's MLP block relative to wave 0's nearest one, in units of the
    # wave-0 sample period (0 = both enter together = they serialise on the matrix pipe and wait for gathers together; 0.5 = one
    # computes while the other gathers)
    print("# phase offset of the partners' MLP entries (fraction of a sample period), samples 0-191 in groups of 16, median over workgroups", file=out)
    rows = []
    for b in used:
        e0 = np.cumsum(np.concatenate([[0], np.diff(t[b, 0].reshape(-1)) & 0xFFFFFFFF]))[9::SLOTS] + t[b, 0, 0, 0]
        e1 = np.cumsum(np.concatenate([[0], np.diff(t[b, 1].reshape(-1)) & 0xFFFFFFFF]))[9::SLOTS] + t[b, 1, 0, 0]
        period = np.median(np.diff(e0))
        off = []
        for x in e1:
            k = np.searchsorted(e0, x, "right") - 1
            off.append(((x - e0[k]) / period) % 1.0 if 0 <= k < len(e0) - 1 else np.nan)
        rows.append(off)
    rows = np.array(rows)
    import warnings
    for g0 in range(0, SAMPLES, 16):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            print(f"  samples {g0:3d}-{g0 + 15:3d}: " + " ".join(f"{np.nanmedian(rows[:, k]):.2f}" for k in range(g0, g0 + 16)), file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--no-build", action="store_true")
    ap.add_argument("--extra", action="append", default=[])
    ap.add_argument("--out", default=None)
    ap.add_argument("--raw", default=None, help="also save the raw stamps as .npy")
    ap.add_argument("--lib", default=LIB, help="an instrumented library built elsewhere (with --no-build)")
    args = ap.parse_args()
    if not args.no_build:
        build(args.extra)
    if args.build_only:
        print("built", LIB)
        return
    os.environ["THERMONERF_HIP_LIB"] = os.path.abspath(args.lib)
    import bench
    from thermo_nerf_amd import _hip

    sys.argv = ["bench.py", "--steps", "1", "--warmup", "1"]
    try:
        bench.main()
    except SystemExit:
        pass
    lib = _hip.load()
    n = BLOCKS * 2 * SAMPLES * SLOTS
    buf = (ctypes.c_uint32 * n)()
    lib.tn_field_stamps_read.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    rc = lib.tn_field_stamps_read(buf, n)
    assert rc == 0, rc
    if args.raw:
        import numpy as np
        np.save(args.raw, np.asarray(buf, dtype=np.uint32))
    out = open(args.out, "w") if args.out else sys.stdout
    print("# tools/field_stamps.py" + (" " + " ".join(args.extra) if args.extra else "") +
          ": bench.py's 800x800 frame at S=192, fp32; stamped build of main_mfma_rays_kernel<true,false>", file=out)
    analyse(buf, out)


if __name__ == "__main__":
    main()
