#!/usr/bin/env python3
"""Times the spherical noise (csrc/noise.hip through ``makani_amd.noise.SphericalNoise``) on one MI355X.

    python3 tools/noise_bench.py [--window 0.1] [--rounds 3] [--out FILE.json]

At 73 channels on the 721 x 1440 equiangular grid (``lmax`` 240, ``mmax`` 241), for the E - 1 perturbed members of ensembles of
E = 4 and 16 (219 and 1095 rows) and for all E members (292 and 1168 rows: an even row count, the 16-byte stores):

* ``coefficients`` with ``phi = 0`` and ``phi = 0.5``: ``MK_NOISE=hip`` against ``MK_NOISE=torch`` (the same call on the same module,
  alternated in one process);
* ``coefficients`` against a plain ``torch.randn`` of the same size scaled by ``sigma_l`` (no reproducible counter, no triangle);
* ``sample`` (the draw and the inverse transform), ``hip`` against ``torch``;
* the kernel alone against its algorithmic bytes, 8 B per coefficient written and 16 B with ``phi > 0``, in TB/s.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths must agree on it within twice the bound of DESIGN section 41 taken at the largest radius a draw can have
(``sqrt(48 ln 2)``).  It fails when no GPU is found.  The default of ``MK_NOISE`` follows DESIGN section 19: ``hip`` only if no row
here is slower than the torch path; the table of DESIGN section 41 is this tool's output.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import timed, window, with_knob  # noqa: E402

C, H, W, LMAX, MMAX = 73, 721, 1440, 240, 241
U, K_COEF = 2.0 ** -24, 12.0
RAD_MAX = math.sqrt(48.0 * math.log(2.0))          # u1 = 2^-24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("noise_bench: no GPU found")
    from makani_amd import ops
    from makani_amd.noise import SphericalNoise, degree_sigmas, power_law_spectrum
    from makani_amd.sht import InverseRealSHT
    dev = torch.device("cuda:0")
    isht = InverseRealSHT(H, W, LMAX, MMAX, "equiangular")
    sig = degree_sigmas(power_law_spectrum(LMAX, 2.0), 1.0, MMAX)
    rows, kernels = [], []
    print(f"{'row':>40} {'E':>3} {'rows':>5} {'hip ms':>10} {'other ms':>10} {'other/hip':>9}")
    for E in (4, 16):
        for n in ((E - 1) * C, E * C):
            mods = {phi: SphericalNoise(isht, sig, seed=7, phi=phi).to(dev) for phi in (0.0, 0.5)}
            # ---- the two paths on this shape, a fresh draw and an AR(1) step, within twice the bound
            lim = 2.0 * K_COEF * U * RAD_MAX * mods[0.0].sigma_l.double().view(LMAX, 1, 1, 1)
            got = {}
            for mode in ("hip", "torch"):
                m = mods[0.5]
                m.reset()
                first = with_knob("MK_NOISE", mode, lambda: m.coefficients(n).clone())()
                got[mode] = (first, with_knob("MK_NOISE", mode, lambda: m.coefficients(n).clone())())
            for k, slack in ((0, 1.0), (1, 2.0)):        # the step carries both draws' bounds and three more roundings
                d = torch.view_as_real(got["hip"][k]).double() - torch.view_as_real(got["torch"][k]).double()
                assert bool((d.abs() <= slack * lim).all()), f"paths disagree: E={E} rows={n} {'AR(1)' if k else 'fresh'}"
            assert bool((got["hip"][0][5, 7:] == 0).all()) and bool(torch.isfinite(torch.view_as_real(got["hip"][1])).all())
            del got, d, lim
            torch.cuda.empty_cache()

            def row(name, fn_hip, fn_other, other):
                t_hip, t_other = timed([fn_hip, fn_other], args.window, args.rounds)
                r = dict(row=name, E=E, rows=n, hip_ms=round(t_hip * 1e3, 4), other=other, other_ms=round(t_other * 1e3, 4),
                         ratio=round(t_other / t_hip, 3))
                rows.append(r)
                print(f"{name:>40} {E:>3} {n:>5} {r['hip_ms']:>10.3f} {r['other_ms']:>10.3f} {r['ratio']:>9.2f}", flush=True)

            for phi, m in mods.items():
                m.reset()
                m.coefficients(n)
                fn = lambda m=m: m.coefficients(n)
                row(f"coefficients, phi = {phi}", with_knob("MK_NOISE", "hip", fn), with_knob("MK_NOISE", "torch", fn), "torch")
            sl = mods[0.0].sigma_l.view(LMAX, 1, 1, 1)
            randn = lambda: torch.randn(LMAX, MMAX, n, 2, device=dev) * sl
            row("coefficients against scaled randn", with_knob("MK_NOISE", "hip", lambda: mods[0.0].coefficients(n)), randn, "randn")
            fn = lambda: mods[0.0].sample(n)
            row("sample", with_knob("MK_NOISE", "hip", fn), with_knob("MK_NOISE", "torch", fn), "torch")
            # ---- the kernel alone
            os.environ["MK_NOISE"] = "hip"
            st = torch.zeros(LMAX, MMAX, n, dtype=torch.complex64, device=dev)
            for phi in (0.0, 0.5):
                fn = lambda: ops.noise_spectrum(st, mods[0.0].sigma_l, 7, t=1, t_dev=mods[0.0].draws, phi=phi)
                for _ in range(2):
                    fn()
                sec = window(fn, 50)
                by = LMAX * MMAX * n * (8 if phi == 0.0 else 16)
                k = dict(kernel=f"mk_noise_spectrum, phi = {phi}", E=E, rows=n, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 3),
                         Gnormals=round(LMAX * (MMAX + 1) / 2 * n * 2 / sec / 1e9, 1))
                kernels.append(k)
                print(f"{'kernel: ' + k['kernel']:>40} {E:>3} {n:>5} {k['ms']:>10.3f} ms {k['TBs']:>6.3f} TB/s (algorithmic), "
                      f"{k['Gnormals']} G normals/s", flush=True)
            del st, mods
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="noise_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["other"] == "torch" and r["ratio"] < 1.0]
    print(f"noise_bench: done, {len(losing)} of {sum(r['other'] == 'torch' for r in rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} E={r['E']} rows={r['rows']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
