#!/usr/bin/env python3
"""One call of the Reed-Solomon outer code (sfe_dsp_reed_*): n_frames interleaved, whitened frames in HBM into payloads,
records and statuses (decode), or payloads into frames (encode).  Three kinds of frames are decoded: clean ones (every
codeword leaves at the ballot of its syndromes), frames with t wrong bytes in every codeword (the whole decoder runs and
patches), and frames whose every byte is wrong (the whole decoder runs and gives up).  256 different frames of a kind are
repeated up to n_frames.
    ours   sfe_dsp_reed_process_stream / sfe_dsp_reed_encode_stream: HIP events, 5 warm-up calls, then 5 windows of as many
           calls as take about 0.1 s (3 to 200): the median window's mean per call, with the fastest and the slowest window
           beside it.  Nothing synchronises inside a window.
    host   the round trip it replaces: copy the input down, sfe_dsp_reed_plan on one host core, copy the output up; wall
           clock, on the call's first min(n_frames, 512) frames, one warm-up then 3 calls, the median, as microseconds per
           frame beside ours.
    share  the bytes the call must move (frame + payload, + 12 of record and status when decoding) over its time, as a share
           of the 6.29 TB/s copy ceiling: how far from memory-bound the call is.
The check column compares the first four frames with the plan's bytes, records and statuses and counts the statuses.
    python scripts/time_reed.py > profiles/reed/time_reed.txt
ROWS="shape:n_frames;..." limits the run to those rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api  # noqa: E402

WARM, WINDOWS, HOST_FRAMES, HOST_REPS, CHECK, KINDS, COPY_CEILING = 5, 5, 512, 3, 4, 256, 6.29e12
SHAPES = {"A": (0x187, 112, 11, 255, 32, 4), "B": (0x11d, 0, 1, 255, 64, 1)}
ROWS = [("A", 1), ("A", 4096), ("A", 65536), ("B", 65536)]
WANT = {(s.split(":")[0], int(s.split(":")[1])) for s in os.environ["ROWS"].split(";")} if os.environ.get("ROWS") else None


def time_calls(run):
    """(median, fastest, slowest) window's mean ms per call, calls per window."""
    t = api.Timer()
    for _ in range(WARM):
        run()
    t.start()
    run()
    t.stop()
    reps = int(min(200, max(3, np.ceil(100.0 / max(t.elapsed_ms(), 1e-3)))))
    ms = []
    for _ in range(WINDOWS):
        t.start()
        for _ in range(reps):
            run()
        t.stop()
        ms.append(t.elapsed_ms() / reps)
    return float(np.median(ms)), min(ms), max(ms), reps


def damaged(frames, shape, kind, rng):
    prim, fcr, step, n, n_par, I = shape
    f = frames.copy()
    if kind == "t wrong":
        for b in range(f.shape[0]):
            for i in range(I):
                at = rng.choice(n, size=n_par // 2, replace=False) * I + i
                f[b, at] ^= rng.integers(1, 256, size=at.size, dtype=np.uint8)
    elif kind == "all wrong":
        f ^= rng.integers(1, 256, size=f.shape, dtype=np.uint8)
    return f


def main():
    lib = api._l.load()
    print("# whitened frames; ms per call; us per frame; the host round trip on the first min(n_frames, %d) frames" % HOST_FRAMES)
    print(f"{'shape':>5s} {'frames':>6s} {'call':>16s} {'ms':>9s} {'min':>8s} {'max':>8s} {'reps':>4s} {'us/frame':>9s} {'GB/s':>8s} {'share':>6s} "
          f"{'host us/frame':>13s} {'x':>8s}   check")
    for key, nf in ROWS:
        if WANT is not None and (key, nf) not in WANT:
            continue
        shape = SHAPES[key]
        rng = np.random.default_rng(nf + ord(key))
        wh = rng.integers(0, 256, size=shape[3] * shape[5], dtype=np.uint8)
        h = api.Reed(*shape, whiten=wh)
        P, Fb = h.payload_bytes, h.frame_bytes
        nk = min(nf, KINDS)
        pay = rng.integers(0, 256, size=(nk, P), dtype=np.uint8)
        clean = h.encode(pay)
        idx = np.arange(nf) % nk
        d_out, d_rec, d_st = api.DeviceArray(nf * P // 4 + 4), api.DeviceArray(2 * nf), api.DeviceArray(nf)
        d_frm = api.DeviceArray(nf * Fb // 4 + 4)
        calls = [(kind, damaged(clean, shape, kind, rng)[idx]) for kind in ("clean", "t wrong", "all wrong")] + [("encode", pay[idx])]
        for kind, data in calls:
            enc = kind == "encode"
            d_in = api.DeviceArray.from_bytes(data)
            run = (lambda: h.encode_stream(d_in, nf, d_frm)) if enc else (lambda: h.process_stream(d_in, nf, d_out, d_rec, d_st))
            ms, lo, hi, reps = time_calls(run)
            api.sync()
            k = min(nf, CHECK)
            if enc:
                got = d_frm.to_numpy().view(np.uint8)[:nf * Fb].reshape(nf, Fb)
                equal = np.array_equal(got[:k], api.reed_plan(*shape, whiten=wh, data=data[:k], encode=True))
                chk = f"first {k} frames {'equal' if equal else 'DIFFER from'} the plan's"
            else:
                by = d_out.to_numpy().view(np.uint8)[:nf * P].reshape(nf, P)
                rec, st = d_rec.to_numpy().view(np.uint32).reshape(nf, 2), d_st.to_numpy().view(np.int32)
                want = api.reed_plan(*shape, whiten=wh, data=data[:k])
                equal = np.array_equal(by[:k], want[0]) and np.array_equal(rec[:k], want[1]) and np.array_equal(st[:k], want[2])
                chk = (f"first {k} frames {'equal' if equal else 'DIFFER from'} the plan's; statuses 0/1/2: "
                       f"{int((st == 0).sum())}/{int((st == 1).sum())}/{int((st == 2).sum())}; bytes corrected {int(rec[:, 0].sum())}")
            hn = min(nf, HOST_FRAMES)
            host = np.empty((hn, data.shape[1]), np.uint8)
            up = np.zeros((hn, Fb if enc else P), np.uint8)

            def round_trip():
                api.check(lib.sfe_dsp_memcpy_d2h(host.ctypes.data, d_in.ptr, host.nbytes, None))
                api.sync()
                res = api.reed_plan(*shape, whiten=wh, data=host, encode=enc)
                up[:] = res if enc else res[0]
                api.check(lib.sfe_dsp_memcpy_h2d((d_frm if enc else d_out).ptr, up.ctypes.data, up.nbytes, None))
                api.sync()
            round_trip()
            ths = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                round_trip()
                ths.append((time.perf_counter() - t0) * 1e3)
            th_us = float(np.median(ths)) * 1e3 / hn
            moved = nf * (P + Fb + (0 if enc else 12))
            rate = moved / (ms * 1e-3)
            print(f"{key:>5s} {nf:6d} {kind:>16s} {ms:9.4f} {lo:8.4f} {hi:8.4f} {reps:4d} {ms * 1e3 / nf:9.4f} {rate / 1e9:8.1f} {100 * rate / COPY_CEILING:5.1f}% "
                  f"{th_us:13.2f} {th_us / (ms * 1e3 / nf):8.1f}   {chk}", flush=True)
            d_in.free()
        h.close()
        for d in (d_out, d_rec, d_st, d_frm):
            d.free()


if __name__ == "__main__":
    main()
