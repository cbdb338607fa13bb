#!/usr/bin/env python3
"""The bulk resampler call with SEVERAL channels at odd strides, in both modes (resample / decimate), over the sweep's rates: every channel against the
oracle -- exact mode bits, default mode within 1e-5 -- and the same output count for every channel; inputs off 16-byte boundaries included."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from simplefe_amd import api, lib, synth  # noqa: E402
from oracle import binding as orc  # noqa: E402

RATES = [(1, 1.0), (1, 2.0), (1, 3.0), (1, 7.0), (1, 64.0), (1, 128.0), (1, 2.5), (1, 1.77), (2, 0.5), (2, 1.5), (3, 5.0 / 3.0), (3, 1.77), (3, 0.77), (4, 1.25), (5, 0.8), (8, 1.0 / 8.0),
         (9, 10.0 / 9.0), (24, 25.0 / 24.0), (32, 1.77)]
bad, tried, worst = {}, 0, 0.0
B = 4096
for (U, rate), plen, cplx, exact, mode, shift in itertools.product(RATES, (7, 32), (True, False), (True, False), ("resample", "decimate"), (0, 1)):
    if mode == "decimate" and (U != 1 or rate < 1.0):
        continue
    rate = float(np.float32(rate))
    taps = synth.lowpass_taps(max(U, plen * U - (U > 1)), 0.9 * min(1.0 / U, 1.0 / max(rate * U, 1.0)), gain=float(U))
    w = 2 if cplx else 1
    nch = 3
    n = 20 * B if rate < 50 else 200 * B
    stride = n + 5 + shift
    x = np.stack([synth.synth_f32(w * n, ch=(tried + c) % 60) for c in range(nch)])
    buf = np.zeros(w * (shift + stride * nch), np.float32)
    for c in range(nch):
        buf[w * (shift + stride * c): w * (shift + stride * c) + w * n] = x[c]
    cap = int(n / rate) + 4 * (n // B) + 64
    tried += 1
    try:
        d = api.DeviceArray.from_numpy(buf)
        d_out = api.DeviceArray(w * (cap + 3) * nch)
        r = api.Rs(taps, U, B, mode=lib.RS_RESAMPLE if mode == "resample" else lib.RS_DECIMATE, data_complex=cplx, n_channels=nch)
        r.set_exact(exact)
        cut = 8 * B
        k1 = r.process_stream(d.ptr + 4 * w * shift, cut, d_out, cap + 3, rate, in_stride=stride, out_stride=cap + 3)
        k2 = r.process_stream(d.ptr + 4 * w * (shift + cut), n - cut, d_out.ptr + 4 * w * k1, cap + 3 - k1, rate, in_stride=stride, out_stride=cap + 3)
        y = d_out.to_numpy().reshape(nch, w * (cap + 3))[:, : w * (k1 + k2)]
        r.close()
        for c, part in itertools.product(range(nch), range(w)):
            ref, _ = (orc.Resample if mode == "resample" else orc.Decimate)(taps, U, B).stream(np.ascontiguousarray(x[c, part::w]), rate)
            got = y[c, part::w]
            key = None
            if len(ref) != len(got):                  # the oracle's total already leaves a pending leftover out: no slack
                key = "output count differs"
            elif exact and not np.array_equal(got.view(np.uint32), ref[: len(got)].view(np.uint32)):
                key = "exact mode: bits differ"
            elif not exact and len(got):
                e = synth.rel_rms(got, ref[: len(got)])
                worst = max(worst, e)
                if not e <= 1e-5:
                    key = "default mode: beyond 1e-5"
            if key:
                bad.setdefault(key, []).append((mode, U, round(rate, 4), plen, cplx, exact, shift, c, len(got), len(ref)))
                break
    except Exception as e:                   # noqa: BLE001
        bad.setdefault(str(e).split(": ", 1)[-1][:110], []).append((mode, U, round(rate, 4), plen, cplx, exact, shift))
print(f"{tried} combinations tried, {sum(len(v) for v in bad.values())} bad; worst default-mode rel-RMS {worst:.2e}")
for k, v in bad.items():
    print(f"-- {len(v):4d} x  {k}")
    for c in v[:12]:
        print("        ", c)
