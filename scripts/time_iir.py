#!/usr/bin/env python3
"""The streaming biquad-cascade IIR filter (sfe_dsp_iir_*) over 2^28 samples generated in HBM by sfe_dsp_synth_fill (u8:
the first 2^29 bytes of the same buffer as (I,Q) pairs; real: its first 2^28 floats), one call per launch: HIP events,
warm-up then 20 timed calls, mean.  bytes = what the two passes move: the input twice and the output once -- 24 B per
cf32 sample, 12 B per u8 or real sample; frac = bytes / time / 6.29 TB/s (the measured copy ceiling).
Beside some rows, what the library could do before: the filter's impulse response truncated where its tail energy falls
below 1e-12 of the total, run through api.Fir over the same cf32 samples (checked against the IIR on a short stream
first; 5 timed calls).  Where Fir refuses the length the row says so.
    python scripts/time_iir.py > profiles/iir/time_iir.txt
LOG2N=24 shortens the stream; FIR=0 leaves the FIR rows out; SHAPES="name:fmt;..." limits the run to those rows (a counter pass)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS = 20
FIR = os.environ.get("FIR", "1") != "0"
n = 1 << int(os.environ.get("LOG2N", "28"))
F = synth.iir_grid_filters()
ROWS = [("dc(0.995)", F["dc(0.995)"], True), ("dc(0.9999)", F["dc(0.9999)"], True), ("butter(4,0.025)", F["butter(4,0.025)"], False),
        ("butter(8,0.1)", synth.iir_butter_lowpass(8, 0.1), True), ("dc(0.999)+butter(8,0.1)", F["dc(0.999)+butter(8,0.1)"], False),
        ("butter(16,0.1)", F["butter(16,0.1)"], False)]


WANT = {tuple(s.rsplit(":", 1)) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None


def truncated_response(sos):
    """The impulse response up to where the energy of what is left falls below 1e-12 of the whole."""
    m = 1 << 12
    while True:
        x = np.zeros(m)
        x[0] = 1.0
        h = synth.iir_reference(x, sos)
        tail = np.cumsum((h * h)[::-1])[::-1]
        if tail[m // 2] < 1e-14 * tail[0]:          # the response is over well inside the window
            return h[:int(np.argmax(tail < 1e-12 * tail[0]))]
        m *= 4


def time_calls(run, reps):
    t = api.Timer()
    for _ in range(3):
        run()
    t.start()
    for _ in range(reps):
        run()
    t.stop()
    return t.elapsed_ms() / reps


def main():
    G = api.iir_plan(F["dc(0.995)"])[0]
    x = api.DeviceArray(2 * n)
    x.fill_synth(synth.SEED)
    y = api.DeviceArray(2 * n)
    print(f"# 2^{n.bit_length() - 1} samples per call, block G = {G}")
    print(f"{'filter':>24s} {'S':>2s} {'in':>5s} {'ms':>8s} {'GB':>6s} {'frac':>6s}   the truncated response through Fir")
    for name, sos, with_fir in ROWS:
        for fmt in ("cf32", "u8", "real"):
            if WANT is not None and (name, fmt) not in WANT:
                continue
            f = api.Iir(sos, data_complex=fmt != "real")
            if fmt == "u8":
                f.set_input_format(lib.FMT_U8)
            ms = time_calls(lambda: f.process_stream(x, n, y), REPS)
            f.close()
            gb = (24 if fmt == "cf32" else 12) * n / 1e9
            note = ""
            if fmt == "cf32" and with_fir and FIR:
                h = truncated_response(sos)
                try:
                    fir = api.Fir(h.astype(np.float32), data_complex=True)
                    xs = synth.synth_cf32(16 * G).view(np.complex64)
                    chk = synth.rel_rms(fir.filter(xs.view(np.float32))[0], api.Iir(sos).filter(xs).view(np.float32))
                    fir.reset()
                    fms = time_calls(lambda: fir.process_stream(x, y, n), 5)
                    fir.close()
                    note = f"   {h.size} taps: {fms:9.3f} ms, {fms / ms:6.1f}x the IIR's (rel-RMS between the two {chk:.1e})"
                except api.SfeError as e:
                    note = f"   {h.size} taps: refused ({e})"
            print(f"{name:>24s} {len(sos):2d} {fmt:>5s} {ms:8.3f} {gb:6.2f} {gb / ms / 6.29:6.3f}{note}", flush=True)
    x.free()
    y.free()


if __name__ == "__main__":
    main()
