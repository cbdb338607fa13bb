#!/usr/bin/env python3
"""One call of the quasi-cyclic LDPC code (sfe_dsp_ldpc_*): n_words codewords of float32 soft values in HBM into payload
bytes, records and statuses (decode), or payload bytes into codeword bytes (encode).  The codes are cases B (n = 648,
Z = 27, four codewords to a workgroup) and F (n = 8192, Z = 512, one) of tests/ldpc_cases.py, scale 8, a = 12, beta = 0,
max_iter = 32.  Three kinds of words are decoded: clean ones (the first syndrome is zero: no iteration), noisy ones at the
case's Eb/N0 (a few iterations each), and hopeless ones at -2 dB (all 32 iterations).  64 different words of a kind are
repeated up to n_words.
    ours   sfe_dsp_ldpc_process_stream / sfe_dsp_ldpc_encode_stream: HIP events, 5 warm-up calls, then 5 windows of as many
           calls as take about 0.1 s (3 to 200): the median window's mean per call, with the fastest and the slowest window
           beside it.  Nothing synchronises inside a window.
    Gbit/s the decoded (or encoded) payload bits over the call's time.
    ns/it  the call's time over the iterations it ran, summed over its codewords ("-" where there were none).
    share  the bytes the call must move (4 n of soft values, ceil(k / 8) and 16 of record and status when decoding;
           ceil(k / 8) + ceil(n / 8) when encoding) over its time, as a share of the 6.29 TB/s copy ceiling.
    host   the round trip it replaces: copy the input down, sfe_dsp_ldpc_plan on one host core, copy the output up; wall
           clock, on the call's first min(n_words, 512) words, one warm-up then 3 calls, the median, as microseconds per
           word beside ours.
The check column compares the first four words with the plan's bytes, records and statuses and counts the statuses.
    python scripts/time_ldpc.py > profiles/ldpc/time_ldpc.txt
ROWS="case:n_words;..." limits the run to those rows."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from simplefe_amd import api  # noqa: E402
import ldpc_cases as lc  # noqa: E402

WARM, WINDOWS, HOST_WORDS, HOST_REPS, CHECK, KINDS, COPY_CEILING = 5, 5, 512, 3, 4, 64, 6.29e12
PARAMS = (lc.SCALE, 12, 0, 32)
ROWS = [("B", 1), ("B", 4096), ("B", 65536), ("F", 1), ("F", 4096), ("F", 65536)]
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


def main():
    lib = api._l.load()
    print("# float32 soft values, scale %g, a = %d, beta = %d, max_iter = %d; ms per call; the host round trip on the first min(n_words, %d) words"
          % (*PARAMS, HOST_WORDS))
    print(f"{'case':>4s} {'words':>6s} {'call':>9s} {'ms':>9s} {'min':>8s} {'max':>8s} {'reps':>4s} {'us/word':>9s} {'Gbit/s':>8s} {'iters':>6s} {'ns/it':>8s} "
          f"{'GB/s':>8s} {'share':>6s} {'host us/word':>12s} {'x':>8s}   check")
    for key, nw in ROWS:
        if WANT is not None and (key, nw) not in WANT:
            continue
        s, Z = lc.CASES[key]
        n, k, kb, nb = lc.sizes(key)
        rng = np.random.default_rng(nw + ord(key))
        t0 = time.perf_counter()
        h = api.Ldpc(s, Z, *PARAMS)
        create_ms = (time.perf_counter() - t0) * 1e3
        nk = min(nw, KINDS)
        pay = rng.integers(0, 256, size=(nk, kb), dtype=np.uint8)
        code = h.encode(pay)
        assert np.array_equal(code[:CHECK], api.ldpc_plan(s, Z, data=pay[:CHECK]))
        tx = (1.0 - 2.0 * np.unpackbits(code, axis=1)[:, :n]).astype(np.float32)
        idx = np.arange(nw) % nk
        d_out, d_rec, d_st = api.DeviceArray(nw * kb // 4 + 4), api.DeviceArray(3 * nw), api.DeviceArray(nw)
        d_code = api.DeviceArray(nw * nb // 4 + 4)
        calls = [("clean", tx), ("noisy", (tx + lc.sigma(key, lc.EBN0[key]) * rng.standard_normal(tx.shape)).astype(np.float32)),
                 ("hopeless", (tx + lc.sigma(key, lc.HOPELESS_DB) * rng.standard_normal(tx.shape)).astype(np.float32)), ("encode", pay)]
        for kind, kinds in calls:
            enc = kind == "encode"
            data = kinds[idx]
            assert data.any() and data.shape == (nw, kb if enc else n)
            d_in = api.DeviceArray.from_bytes(data) if enc else api.DeviceArray.from_numpy(data)
            run = (lambda: h.encode_stream(d_in, nw, d_code)) if enc else (lambda: h.process_stream(d_in, nw, d_out, d_rec, d_st))
            ms, lo, hi, reps = time_calls(run)
            api.sync()
            c = min(nw, CHECK)
            iters = 0
            if enc:
                got = d_code.to_numpy().view(np.uint8)[:nw * nb].reshape(nw, nb)
                equal = np.array_equal(got[:c], api.ldpc_plan(s, Z, data=data[:c]))
                chk = f"first {c} words {'equal' if equal else 'DIFFER from'} the plan's"
            else:
                by = d_out.to_numpy().view(np.uint8)[:nw * kb].reshape(nw, kb)
                rec, st = d_rec.to_numpy(3 * nw).view(np.uint32).reshape(nw, 3), d_st.to_numpy(nw).view(np.int32)
                want = api.ldpc_plan(s, Z, *PARAMS, x=data[:c])
                equal = np.array_equal(by[:c], want[0]) and np.array_equal(rec[:c], want[1]) and np.array_equal(st[:c], want[2])
                iters = int(rec[:, 0].sum())
                chk = (f"first {c} words {'equal' if equal else 'DIFFER from'} the plan's; statuses 0/1/3: "
                       f"{int((st == 0).sum())}/{int((st == 1).sum())}/{int((st == 3).sum())}; payloads back {int((by == lc.payload_bits_only(key, pay)[idx]).all(axis=1).sum())}")
            hn = min(nw, HOST_WORDS)
            host = np.empty((hn, data.shape[1]), data.dtype)
            up = np.zeros((hn, nb if enc else kb), np.uint8)

            def round_trip():
                api.check(lib.sfe_dsp_memcpy_d2h(host.ctypes.data, d_in.ptr, host.nbytes, None))
                api.sync()
                up[:] = api.ldpc_plan(s, Z, data=host) if enc else api.ldpc_plan(s, Z, *PARAMS, x=host)[0]
                api.check(lib.sfe_dsp_memcpy_h2d((d_code if enc else d_out).ptr, up.ctypes.data, up.nbytes, None))
                api.sync()
            round_trip()
            ths = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                round_trip()
                ths.append((time.perf_counter() - t0) * 1e3)
            th_us = float(np.median(ths)) * 1e3 / hn
            moved = nw * ((kb + nb) if enc else (4 * n + kb + 16))
            rate = moved / (ms * 1e-3)
            per_it = f"{ms * 1e6 / iters:8.1f}" if iters else f"{'-':>8s}"
            print(f"{key:>4s} {nw:6d} {kind:>9s} {ms:9.4f} {lo:8.4f} {hi:8.4f} {reps:4d} {ms * 1e3 / nw:9.4f} {nw * k / (ms * 1e-3) / 1e9:8.2f} "
                  f"{iters / nw:6.2f} {per_it} {rate / 1e9:8.1f} {100 * rate / COPY_CEILING:5.1f}% {th_us:12.2f} {th_us / (ms * 1e3 / nw):8.1f}   {chk}",
                  flush=True)
            d_in.free()
            del data
        print(f"# case {key}: create (the base matrix checked, its parity part inverted on the host, the tables uploaded) took {create_ms:.1f} ms", flush=True)
        h.close()
        for d in (d_out, d_rec, d_st, d_code):
            d.free()


if __name__ == "__main__":
    main()
