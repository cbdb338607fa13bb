#!/usr/bin/env python3
"""One call of the frame check (sfe_dsp_crc_*): n_frames payloads in HBM into scrambled frames with their CRC behind them
(append), or channel frames into payloads, records and statuses (check).  CRC-32/ISO-HDLC with the CCSDS randomiser, and
without a scrambler on the first shape.  256 different rows are repeated up to n_frames.
    ours   sfe_dsp_crc_append_stream / sfe_dsp_crc_check_stream: HIP events, 5 warm-up calls, then 5 windows of as many calls
           as take about 0.1 s (3 to 200): the median window's mean per call, with the fastest and the slowest window beside it.
           Nothing synchronises inside a window.
    floor  the bytes the call must move (payload + frame, + 12 of record and status when checking) at the 6.29 TB/s copy
           ceiling, computed, in ms; share: the floor over ours.
    host   the round trip it replaces: copy the rows down, zlib.crc32 per frame (and numpy's xor with the sequence where there
           is a scrambler), copy the statuses (check) or the frames (append) up; wall clock, on the call's first
           min(n_frames, 4096) frames, one warm-up then 3 calls, the median, as microseconds per frame beside ours.
    torch  the same law composed in torch on the device: per byte position a table gather and two bit operations over all
           frames (r = table[(r ^ b) & 255] ^ (r >> 8)), the scrambler's xor and the tail's four bytes; on min(n_frames, 4096)
           frames of at most 4096 bytes (a loop over the byte positions: a long row is not run), ms per call scaled to the
           call's frames.
The check column compares the first four frames with the plan's bytes, records and statuses and counts the statuses.
    python scripts/time_crc.py > profiles/crc/time_crc.txt
ROWS="P:n_frames;..." limits the run to those rows."""
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api  # noqa: E402

WARM, WINDOWS, HOST_FRAMES, HOST_REPS, CHECK, KINDS, COPY_CEILING = 5, 5, 4096, 3, 4, 256, 6.29e12
TORCH_FRAMES, TORCH_BYTES = 4096, 4096
HDLC = (32, 0x04C11DB7, 0xFFFFFFFF, 1, 0xFFFFFFFF)
CCSDS, NONE = (8, 0xA9, 0xFF), (0, 0, 0)
# (payload bytes, frames, scrambler)
ROWS = [(1020, 65536, CCSDS), (1020, 65536, NONE), (512, 65536, CCSDS), (1024, 1024, CCSDS), (1 << 20, 1, CCSDS), (1020, 1, CCSDS)]
WANT = {(int(s.split(":")[0]), int(s.split(":")[1])) for s in os.environ["ROWS"].split(";")} if os.environ.get("ROWS") else None


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


def torch_ms(P, nf, pn, check):
    """The law composed in torch, ms per call scaled to nf frames; None where torch is absent or the row too long."""
    try:
        import torch
    except ImportError:
        return None
    if P > TORCH_BYTES or not torch.cuda.is_available():
        return None
    n = min(nf, TORCH_FRAMES)
    dev = torch.device("cuda")
    entries = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
        entries.append(c)
    table = torch.tensor(entries, dtype=torch.int64, device=dev)
    Fb = P + 4
    seq = torch.tensor(api.pn_bytes(*pn, Fb).astype(np.int64) if pn[0] else np.zeros(Fb, np.int64), device=dev)
    rows = torch.randint(0, 256, (n, Fb if check else P), dtype=torch.int64, device=dev)

    def run():
        r = rows ^ seq[None, :rows.shape[1]] if check else rows
        c = torch.full((n,), 0xFFFFFFFF, dtype=torch.int64, device=dev)
        for j in range(P):
            c = table[(c ^ r[:, j]) & 255] ^ (c >> 8)
        c = c ^ 0xFFFFFFFF
        tail = torch.stack([(c >> (8 * k)) & 255 for k in range(4)], dim=1)
        if check:
            return (tail != r[:, P:]).any(dim=1).to(torch.int32), r[:, :P].to(torch.uint8)
        return (torch.cat([r, tail], dim=1) ^ seq[None, :]).to(torch.uint8)
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)) * nf / n


def main():
    lib = api._l.load()
    print("# CRC-32/ISO-HDLC; ms per call; us per frame; the host round trip and torch on the first min(n_frames, %d) frames, scaled" % HOST_FRAMES)
    print(f"{'P':>8s} {'frames':>6s} {'pn':>5s} {'call':>7s} {'ms':>9s} {'min':>8s} {'max':>8s} {'reps':>4s} {'us/frame':>9s} {'GB/s':>8s} {'floor ms':>9s} "
          f"{'share':>6s} {'host us/frame':>13s} {'x':>8s} {'torch ms':>9s} {'x':>7s}   check")
    for P, nf, pn in ROWS:
        if WANT is not None and (P, nf) not in WANT:
            continue
        shape = (*HDLC, *pn, P)
        rng = np.random.default_rng(P + nf)
        h = api.Crc(*shape)
        Fb = h.frame_bytes
        nk = min(nf, KINDS)
        pay = rng.integers(0, 256, size=(nk, P), dtype=np.uint8)
        idx = np.arange(nf) % nk
        frames = api.crc_plan(*shape, data=pay)
        frames[1 % nk, P // 2] ^= 4                                  # one frame of the 256 is wrong
        seq = api.pn_bytes(*pn, Fb) if pn[0] else None
        d_out, d_rec, d_st = api.DeviceArray(nf * P // 4 + 4), api.DeviceArray(2 * nf), api.DeviceArray(nf)
        d_frm = api.DeviceArray(nf * Fb // 4 + 4)
        for kind, data in (("append", pay[idx]), ("check", frames[idx])):
            chk = kind == "check"
            d_in = api.DeviceArray.from_bytes(data)
            run = (lambda: h.check_stream(d_in, nf, d_out, d_rec, d_st)) if chk else (lambda: h.append_stream(d_in, nf, d_frm))
            ms, lo, hi, reps = time_calls(run)
            api.sync()
            k = min(nf, CHECK)
            if chk:
                by = d_out.to_numpy().view(np.uint8)[:nf * P].reshape(nf, P)
                rec, st = d_rec.to_numpy().view(np.uint32).reshape(nf, 2), d_st.to_numpy().view(np.int32)
                want = api.crc_plan(*shape, data=data[:k], verify=True)
                equal = np.array_equal(by[:k], want[0]) and np.array_equal(rec[:k], want[1]) and np.array_equal(st[:k], want[2])
                note = (f"first {k} frames {'equal' if equal else 'DIFFER from'} the plan's; statuses 0/1/2: "
                        f"{int((st == 0).sum())}/{int((st == 1).sum())}/{int((st == 2).sum())}")
            else:
                got = d_frm.to_numpy().view(np.uint8)[:nf * Fb].reshape(nf, Fb)
                equal = np.array_equal(got[:k], api.crc_plan(*shape, data=data[:k]))
                note = f"first {k} frames {'equal' if equal else 'DIFFER from'} the plan's"
            hn = min(nf, HOST_FRAMES)
            host = np.empty((hn, data.shape[1]), np.uint8)
            up_st, up_frm = np.zeros(hn, np.int32), np.zeros((hn, Fb), np.uint8)

            def round_trip():
                api.check(lib.sfe_dsp_memcpy_d2h(host.ctypes.data, d_in.ptr, host.nbytes, None))
                api.sync()
                r = host ^ seq[None, :host.shape[1]] if (chk and seq is not None) else host
                crcs = np.array([zlib.crc32(row[:P].tobytes()) for row in r], np.uint32)
                if chk:
                    up_st[:] = crcs != r[:, P:].copy().view("<u4").ravel()
                    api.check(lib.sfe_dsp_memcpy_h2d(d_st.ptr, up_st.ctypes.data, up_st.nbytes, None))
                else:
                    up_frm[:, :P] = r
                    up_frm[:, P:] = crcs.astype("<u4").view(np.uint8).reshape(hn, 4)
                    if seq is not None:
                        up_frm[:] ^= seq[None, :]
                    api.check(lib.sfe_dsp_memcpy_h2d(d_frm.ptr, up_frm.ctypes.data, up_frm.nbytes, None))
                api.sync()
            round_trip()
            ths = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                round_trip()
                ths.append((time.perf_counter() - t0) * 1e3)
            th_us = float(np.median(ths)) * 1e3 / hn
            moved = nf * (P + Fb + (12 if chk else 0))
            rate, floor = moved / (ms * 1e-3), moved / COPY_CEILING * 1e3
            tm = torch_ms(P, nf, pn, chk)
            print(f"{P:8d} {nf:6d} {('CCSDS' if pn[0] else 'none'):>5s} {kind:>7s} {ms:9.4f} {lo:8.4f} {hi:8.4f} {reps:4d} {ms * 1e3 / nf:9.4f} {rate / 1e9:8.1f} "
                  f"{floor:9.4f} {100 * floor / ms:5.1f}% {th_us:13.2f} {th_us / (ms * 1e3 / nf):8.1f} "
                  + (f"{tm:9.3f} {tm / ms:7.1f}" if tm is not None else f"{'-':>9s} {'-':>7s}") + f"   {note}", flush=True)
            d_in.free()
        h.close()
        for d in (d_out, d_rec, d_st, d_frm):
            d.free()


if __name__ == "__main__":
    main()
