#!/usr/bin/env python3
"""One call of the burst modulator (sfe_dsp_mod_*): n_bursts payloads in HBM -- K = 7 rate-1/2 terminated bursts, BPSK behind
a 32-symbol QPSK preamble, a raised-cosine pulse of Q taps per arm -- into one stream of n_bursts frames that touch
(start_step = F), cf32 or the transmit wire format:
    ours   sfe_dsp_mod_process_stream: HIP events, 10 warm-up calls, then 5 windows of 50 calls each: the median window's
           mean per call, with the fastest and the slowest window beside it.  Nothing synchronises inside a window.
           GB/s and the share of the 6.29 TB/s copy ceiling count the bytes STORED (8 per sample, or 2.5).
Beside each row, in the same process, the two compositions it replaces:
    fir    what the library offered before: sfe_dsp_vit_encode and the symbol map on the host, the symbols zero-stuffed to
           the sample rate, uploaded, and one Fir stream call with the same taps (its fused TX10 store for the wire
           format); wall clock from the payload bytes on the host to the finished stream, one warm-up then 3 calls, median
           and range.  Its samples are compared with the block's (a transform-domain filter: a tolerance, not equality).
    torch  the same law composed of torch-ROCm tensor operations on the device: the bits unpacked, the encoder as a
           windowed parity, the map, the preamble, then one batched matrix product of the symbols' Q-windows with the
           (Q, sps) arms, and for the wire format the quantiser and the packing; HIP events, 2 warm-up calls, then 3 windows
           of 3 calls.  Compared with the block's samples likewise.
The check column compares the first eight frames with sfe_dsp_mod_plan's, for equality.
    python scripts/time_mod.py > profiles/mod/time_mod.txt
TORCH=0 leaves the torch composition out; FIR=0 the host composition; SHAPES="sps:Q:N:n_bursts:tx10;..." limits the rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, synth  # noqa: E402
from simplefe_amd import lib as _l  # noqa: E402

WARM, WINDOWS, REPS, TORCH_WARM, TORCH_WINDOWS, TORCH_REPS, HOST_REPS, CHECK = 10, 5, 50, 2, 3, 3, 3, 8
TORCH = os.environ.get("TORCH", "1") != "0"
FIR = os.environ.get("FIR", "1") != "0"
K, GEN, LP, AMP, CEILING = 7, (0o171, 0o133), 32, 0.5, 6.29e12
SHAPES = [(10, 17, 256, 1, 0), (10, 17, 256, 4096, 0), (10, 17, 256, 4096, 1), (4, 16, 4096, 256, 0), (50, 12, 1024, 256, 0),
          (50, 12, 1024, 256, 1), (10, 64, 256, 4096, 0)]
WANT = {tuple(int(v) for v in s.split(":")) for s in os.environ["SHAPES"].split(";")} if os.environ.get("SHAPES") else None


def time_calls(run, warm, windows, reps):
    """(median, fastest, slowest) window's mean ms per call."""
    t = api.Timer()
    for _ in range(warm):
        run()
    ms = []
    for _ in range(windows):
        t.start()
        for _ in range(reps):
            run()
        t.stop()
        ms.append(t.elapsed_ms() / reps)
    return float(np.median(ms)), min(ms), max(ms)


class _Cai:
    """A window of a DeviceArray for torch.as_tensor (the CUDA array interface, which torch-ROCm reads too)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def torch_law(torch, B, pre, taps, sps, Q, n_info, tx10):
    """The law on a (n_bursts, n_bytes) uint8 tensor: the stream of touching frames, (n_bursts F, 2) float32 or its bytes."""
    nb, dev = B.shape[0], B.device
    sh = torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)
    bits = ((B[:, :, None] >> sh) & 1).reshape(nb, -1)[:, :n_info].float()
    u = torch.nn.functional.pad(bits, (K - 1, K - 1))                    # u_t = 0 before the payload and in the tail
    win = u.unfold(1, K, 1)                                               # (nb, T, K): win[t, i] = u_(t - (K-1) + i)
    g = torch.tensor([[(gj >> (K - 1 - i)) & 1 for gj in GEN] for i in range(K)], dtype=torch.float32, device=dev)
    coded = torch.remainder(win @ g, 2.0).reshape(nb, -1)                 # (nb, T n) in the order of (t, j)
    data = AMP * (1.0 - 2.0 * coded)
    s = torch.stack([torch.cat([pre[:, 0].expand(nb, -1), data], 1), torch.cat([pre[:, 1].expand(nb, -1), torch.zeros_like(data)], 1)], 1)
    w = torch.nn.functional.pad(s, (Q - 1, Q - 1)).unfold(2, Q, 1)        # (nb, 2, N + Q - 1, Q): w[k, i] = s[k - (Q-1) + i]
    y = (w @ taps).permute(0, 2, 3, 1).reshape(-1, 2)                     # arms (Q, sps) flipped in q: (nb, 2, N+Q-1, sps)
    if not tx10:
        return y.contiguous()
    q = (((y * 511.0).to(torch.int32).to(torch.int16).to(torch.int32) + 512) & 0x3FF).reshape(-1, 4)
    hi = (q[:, 0] >> 8) | ((q[:, 1] >> 8) << 2) | ((q[:, 2] >> 8) << 4) | ((q[:, 3] >> 8) << 6)
    return torch.cat([hi[:, None], q & 0xFF], 1).to(torch.uint8)


def main():
    torch = None
    if TORCH:
        import torch
        print(f"# torch {torch.__version__}")
    print("# K = 7 rate 1/2 terminated, BPSK behind a 32-symbol preamble, raised-cosine pulse; frames touch; ms per call; bytes stored")
    print(f"{'sps':>3s} {'Q':>2s} {'N':>5s} {'bursts':>6s} {'fmt':>4s} {'samples':>9s} {'ms':>9s} {'min':>8s} {'max':>8s} {'GB/s':>7s} {'ceiling':>7s} "
          f"{'fir ms':>9s} {'min':>8s} {'max':>8s} {'x':>7s} {'torch ms':>9s} {'min':>8s} {'max':>8s} {'x':>7s}   check")
    lib = api._l.load()
    for sps, Q, N, nb, tx10 in SHAPES:
        if WANT is not None and (sps, Q, N, nb, tx10) not in WANT:
            continue
        n_info = (N - LP) // 2 - (K - 1)
        n_taps = (Q - 1) * sps + 1
        taps = synth.raised_cosine((np.arange(n_taps) - (n_taps - 1) / 2.0) / sps).astype(np.float32)
        pre = synth.psk_symbols(LP, 4, seed=synth.SEED + 3).astype(np.complex64)
        fmt = _l.FMT_TX10 if tx10 else _l.FMT_F32
        h = api.Mod(K, GEN, n_info, taps, sps, preamble=pre, amp=AMP, out_fmt=fmt)
        assert h.n_sym == N
        F = h.frame_len
        n_out = nb * F
        out_bytes = n_out // 2 * 5 if tx10 else 8 * n_out
        data = np.random.default_rng(synth.SEED + nb).integers(0, 256, size=(nb, h.n_bytes), dtype=np.uint8)
        d_data, d_out = api.DeviceArray.from_bytes(data), api.DeviceArray((out_bytes + 3) // 4)
        ms, lo, hi = time_calls(lambda: h.process_stream(d_data, nb, d_out, n_out, 0, F), WARM, WINDOWS, REPS)
        api.sync()
        got = d_out.to_numpy().view(np.uint8)[:out_bytes]
        k = min(nb, CHECK)
        want = api.mod_plan(K, GEN, n_info, taps, sps, preamble=pre, amp=AMP, out_fmt=fmt, data=data[:k], n_out=k * F, start_step=F)
        equal = np.array_equal(got[:want.nbytes], want.view(np.uint8))
        chk = f"first {k} frames {'equal' if equal else 'DIFFER from'} the plan's"
        h.close()
        ours = got if tx10 else got.view(np.float32)

        def compare(other):
            if tx10:
                return f"{int((np.abs(synth.tx10_unpack(other) - synth.tx10_unpack(ours)) > 1.5 / 511).sum())} values off by more than one step"
            return f"max |d| {float(np.abs(other - ours).max()):.2e}"

        fnote = f"{'':>9s} {'':>8s} {'':>8s} {'':>7s}"
        if FIR:
            try:
                f = api.Fir(taps, data_complex=True)
                if tx10:
                    f.set_output_format(_l.FMT_TX10)
                d_sym, d_fir = api.DeviceArray(2 * n_out), api.DeviceArray((out_bytes + 3) // 4)
                stuffed = np.zeros((nb, F), np.complex64)

                def compose():
                    for b in range(nb):
                        coded = api.vit_encode(K, GEN, np.unpackbits(data[b])[:n_info])
                        stuffed[b, :N * sps:sps] = synth.mod_symbols(coded, 2, AMP, pre)
                    api.check(lib.sfe_dsp_memcpy_h2d(d_sym.ptr, stuffed.ctypes.data, stuffed.nbytes, None))
                    f.reset()
                    f.process_stream(d_sym, d_fir, n_out)
                    api.sync()
                compose()
                ths = []
                for _ in range(HOST_REPS):
                    t0 = time.perf_counter()
                    compose()
                    ths.append((time.perf_counter() - t0) * 1e3)
                th = float(np.median(ths))
                fnote = f"{th:9.3f} {min(ths):8.3f} {max(ths):8.3f} {th / ms:7.1f}"
                other = d_fir.to_numpy().view(np.uint8)[:out_bytes]
                chk += "; fir: " + compare(other if tx10 else other.view(np.float32))
                f.close()
                d_sym.free()
                d_fir.free()
            except Exception as e:
                fnote = f"{'n/a':>9s} {'':>8s} {'':>8s} {'':>7s}"
                chk += f"; fir: {type(e).__name__}: {str(e)[:60]}"

        tnote = f"{'':>9s} {'':>8s} {'':>8s} {'':>7s}"
        if torch is not None:
            try:
                dev = torch.device("cuda:0")
                B = torch.as_tensor(_Cai(d_data.ptr, data.shape, "|u1"), device=dev)
                tp = torch.as_tensor(AMP * pre.view(np.float32).reshape(LP, 2), device=dev)
                arms = np.zeros((Q, sps), np.float32)
                arms.ravel()[:n_taps] = taps
                tt = torch.as_tensor(np.ascontiguousarray(arms[::-1]), device=dev)
                last = []

                def run():
                    last[:] = [torch_law(torch, B, tp, tt, sps, Q, n_info, tx10)]
                tm, tlo, thi = time_calls(run, TORCH_WARM, TORCH_WINDOWS, TORCH_REPS)
                torch.cuda.synchronize()
                tnote = f"{tm:9.3f} {tlo:8.3f} {thi:8.3f} {tm / ms:7.1f}"
                chk += "; torch: " + compare(last[0].cpu().numpy().ravel())
                del B, last
                torch.cuda.empty_cache()
            except Exception as e:
                tnote = f"{'n/a':>9s} {'':>8s} {'':>8s} {'':>7s}"
                chk += f"; torch: {type(e).__name__}: {str(e)[:60]}"
        rate = out_bytes / (ms * 1e-3)
        print(f"{sps:3d} {Q:2d} {N:5d} {nb:6d} {'tx10' if tx10 else 'f32':>4s} {n_out:9d} {ms:9.4f} {lo:8.4f} {hi:8.4f} {rate / 1e9:7.1f} {100 * rate / CEILING:6.1f}% "
              f"{fnote} {tnote}   {chk}", flush=True)
        d_data.free()
        d_out.free()


if __name__ == "__main__":
    main()
