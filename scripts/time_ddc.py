#!/usr/bin/env python3
"""The down-converter bank (sfe_dsp_ddc_*) over 2^28 input samples generated in HBM by sfe_dsp_synth_fill (u8: the first
2^29 bytes of the same buffer as (I,Q) pairs; real: its first 2^28 floats), one call per launch, P = 16 taps per branch,
beside the library composition a user has without it in the same process: per tuning a complex-tap sfe_dsp_fir call at
the full rate, every D-th output gathered and the lead factor applied in torch (u8 input converted by
sfe_dsp_rx_u8_to_f32 first); and for K = 1 the torch composition (mix, conv1d with stride D).  HIP events, warm-up then
20 timed calls (3 for the compositions), mean.
bytes = input (8, 2 or 4 B per sample) + 8 K / D B per input sample; FMA = 4 K P per input sample (complex data) or 2 K P
(real); frac = the larger of bytes / 8 TB/s and 2 FMA / 157.3 TFLOP/s over the time, `bound` names which.
    python scripts/time_ddc.py > profiles/ddc/time_ddc.txt
SHAPES=64:8:cf32,... limits the run to those (D:K:fmt) shapes; COMPOSE=0 leaves both compositions out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

REPS = 20
P = 16
HBM, FP32 = 8.0e12, 157.3e12
COMPOSE = os.environ.get("COMPOSE", "1") != "0"
n = 1 << int(os.environ.get("LOG2N", "28"))
SHAPES = [(D, K, fmt) for D, K in ((4, 1), (4, 4), (10, 1), (10, 8), (64, 1), (64, 8), (64, 64), (500, 1), (500, 8), (500, 64))
          for fmt in ("cf32", "u8")]
SHAPES += [(D, K, "real") for D, K in ((10, 1), (10, 8), (64, 1), (64, 8))]
if os.environ.get("SHAPES"):
    want = {tuple(s.split(":")) for s in os.environ["SHAPES"].split(",")}
    SHAPES = [s for s in SHAPES if (str(s[0]), str(s[1]), s[2]) in want]


def freqs_of(K):
    return np.linspace(-0.45, 0.45, K) + 0.0123 if K > 1 else np.array([0.1234])


def lead(torch, m, D, inc, dev):
    """exp(-j 2 pi ((m D) inc mod 2^32) / 2^32) for the call's outputs m (the composition's phase correction)."""
    ph = (m * D * inc) % (1 << 32)
    a = ph.to(torch.float64) * (-2.0 * np.pi / 2.0 ** 32)
    return torch.polar(torch.ones_like(a), a).to(torch.complex64)


def main():
    import torch
    dev = torch.device("cuda:0")
    L = lib.load()
    x = api.DeviceArray(2 * n)
    x.fill_synth(synth.SEED)
    xf = torch.empty(2 * n, dtype=torch.float32, device=dev)            # the composition's cf32 input (u8 converted)
    full = torch.empty(2 * n, dtype=torch.float32, device=dev)          # one tuning's full-rate FIR output
    t = api.Timer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def event_ms(fn, reps):
        for _ in range(1):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    print(f"# 2^{n.bit_length() - 1} input samples per call, P = {P}; torch {torch.__version__}; frac = larger of bytes / 8 TB/s "
          f"and 2 FMA / 157.3 TFLOP/s over the time")
    print(f"{'D':>4s} {'K':>3s} {'in':>5s} {'ms':>8s} {'GB':>6s} {'GFMA':>7s} {'frac':>6s} {'bound':>5s} {'lib ms':>9s} {'x':>6s} "
          f"{'torch ms':>9s} {'x':>6s}")
    for D, K, fmt in SHAPES:
        h = synth.lowpass_taps(P * D, 0.5 / D)
        f = freqs_of(K)
        dd = api.Ddc(h, D, f, data_complex=fmt != "real")
        if fmt == "u8":
            dd.set_input_format(lib.FMT_U8)
        nd = n // D * D                                                 # whole outputs: 2^28 rounded down to a multiple of D
        n_out = nd // D
        y = api.DeviceArray(2 * K * n_out)
        for _ in range(5):
            dd.process_stream(x, nd, y)
        t.start()
        for _ in range(REPS):
            dd.process_stream(x, nd, y)
        t.stop()
        ms = t.elapsed_ms() / REPS
        dd.close()
        y.free()
        isz = {"cf32": 8, "u8": 2, "real": 4}[fmt]
        gb = (isz * nd + 8.0 * K * n_out) / 1e9
        fma = (4 if fmt != "real" else 2) * K * P * nd
        t_b, t_f = gb * 1e9 / HBM * 1e3, 2.0 * fma / FP32 * 1e3
        frac, bound = max(t_b, t_f) / ms, ("hbm" if t_b >= t_f else "fp32")
        line = f"{D:4d} {K:3d} {fmt:>5s} {ms:8.3f} {gb:6.2f} {fma / 1e9:7.1f} {frac:6.3f} {bound:>5s}"
        if not COMPOSE:
            print(line, flush=True)
            continue
        # the library composition: K complex-tap FIRs at the full rate, strided gather, lead rotation
        incs = synth.ddc_incs(f)
        m = torch.arange(n_out, dtype=torch.int64, device=dev)
        firs = []
        for inc in incs:
            g = (h.astype(np.float64) * np.conj(synth._ddc_phase(np.arange(h.size), inc))).astype(np.complex64)
            firs.append(api.Fir(g, data_complex=fmt != "real"))
        out = torch.empty((K, n_out), dtype=torch.complex64, device=dev)

        def composed():
            src = x.ptr
            if fmt == "u8":
                api.check(L.sfe_dsp_rx_u8_to_f32(x.ptr, xf.data_ptr(), 2 * n, None))
                src = xf.data_ptr()
            for k in range(K):
                firs[k].process_stream(src, full.data_ptr(), nd)
                z = torch.view_as_complex(full[: 2 * nd].view(nd, 2))[::D]
                out[k] = z * lead(torch, m, D, incs[k], dev)
        cms = event_ms(composed, 3)
        for fr in firs:
            fr.close()
        line += f" {cms:9.3f} {cms / ms:6.1f}"
        if K == 1:
            ht = torch.from_numpy(h.astype(np.float32)).to(dev).flip(0).view(1, 1, -1)

            def torch_ddc():
                i = torch.arange(nd, dtype=torch.int64, device=dev)
                if fmt == "u8":
                    v = xu.float().sub_(128.0).mul_(1.0 / 127.0)
                    xc = torch.view_as_complex(v.view(nd, 2))
                elif fmt == "real":
                    xc = xr.to(torch.complex64)
                else:
                    xc = torch.view_as_complex(xt.view(nd, 2))
                z = xc * lead(torch, i, 1, incs[0], dev)
                zr = torch.view_as_real(z).T.contiguous().view(2, 1, nd)                   # re, im as a batch of 2
                zr = torch.nn.functional.pad(zr, (h.size - 1, 0))
                return torch.nn.functional.conv1d(zr, ht, stride=D)
            xu = torch.randint(0, 256, (2 * nd,), dtype=torch.uint8, device=dev) if fmt == "u8" else None
            xr = torch.randn(nd, device=dev) if fmt == "real" else None
            xt = torch.randn(2 * nd, device=dev) if fmt == "cf32" else None
            tms = event_ms(torch_ddc, 3)
            del xu, xr, xt
            torch.cuda.empty_cache()
            line += f" {tms:9.3f} {tms / ms:6.1f}"
        print(line, flush=True)
    x.free()


if __name__ == "__main__":
    main()
