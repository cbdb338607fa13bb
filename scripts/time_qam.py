#!/usr/bin/env python3
"""The QAM mapper and soft demapper (sfe_dsp_qam_*) at the OFDM receiver's shapes of the README: the data symbols of
(N, cp, T, Ns, n_bursts) = (256, 32, 2, 14, 16 384) -- rows of 14 x 196 symbols -- and (4096, 288, 1, 14, 1024) -- rows of
14 x 3136 -- 44.96 M symbols a call either way.  map and demap at M = 16, 64 and 256; demap with and without CSI (csi_period =
Nd, csi_len = N, the data bins' FFT bins); both with and without a random perm.  Beside every row:
  torch  the same law composed in torch on tensors that hold the same bytes -- per axis (y[..., None] - lev)^2, the two masked
         minima per bit, w (D1 - D0), a scatter through perm; map: the bits unpacked, gathered through perm, the words looked up
         -- in chunks of rows that keep its temporaries below 2 GiB.  It is held to the block (demap: 1e-5 of the largest
         value; map: equality) over the first rows before anything is timed.
  frac   bytes / time / 6.29 TB/s, the measured copy ceiling; bytes = 8 + 4 bps per symbol (demap; + 4 per soft value and
         symbol-bit with perm, the table's read; the csi row's read is 8 N per row, counted) and bps / 8 + 8 (map; + 4 bps
         with perm).
Times: device events around WINDOW consecutive calls behind a warm-up, the median of ROUNDS windows.
    python scripts/time_qam.py > profiles/qam/time_qam.txt
ROWS_DIV=16 shortens the calls."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplefe_amd import api, lib, synth  # noqa: E402

ROUNDS, WINDOW = 5, 10
ROWS_DIV = int(os.environ.get("ROWS_DIV", "1"))
SHAPES = [(256, 14, 16384), (4096, 14, 1024)]
ORDERS = (16, 64, 256)
CEILING = 6.29e12


def data_bins(N):
    """The data bins of scripts/time_ofdm.py's shapes: |f| <= 7 N / 16 without DC, every eighth of them a pilot."""
    k = np.arange(N)
    f = np.where(k < N // 2, k, k - N)
    kind = np.where((np.abs(f) <= (N * 7) // 16) & (f != 0), 1, 0)
    kind[(kind == 1) & (np.abs(f) % 8 == 4)] = 2
    return np.flatnonzero(kind == 1).astype(np.uint32)


def torch_demap(torch, z, lev, wbits, scale, csi, idx, perm, out, chunk):
    """z (R, n) complex64, csi (R, N) complex64 or None -> out (R, n bps) float32."""
    m = wbits.shape[1]
    one = [wbits[:, c] == 1 for c in range(m)]
    for a in range(0, z.shape[0], chunk):
        zz = z[a:a + chunk]
        if csi is None:
            w = scale
        else:
            h = csi[a:a + chunk][:, idx]
            w = scale * (h.real * h.real + h.imag * h.imag)
        parts = []
        for y in (zz.real, zz.imag):
            e = (y.unsqueeze(-1) - lev) ** 2
            for c in range(m):
                parts.append(w * (e[..., one[c]].amin(dim=-1) - e[..., ~one[c]].amin(dim=-1)))
        r = torch.stack(parts, dim=-1).reshape(zz.shape[0], -1)
        if perm is None:
            out[a:a + chunk] = r
        else:
            out[a:a + chunk].index_copy_(1, perm, r)


def torch_map(torch, by, lev_of_word, bps, perm, n_sym, out, chunk):
    """by (R, bytes) uint8 -> out (R, n_sym) complex64."""
    m = bps // 2
    shifts = torch.arange(7, -1, -1, device=by.device, dtype=torch.uint8)
    wt = (1 << torch.arange(m - 1, -1, -1, device=by.device)).to(torch.int64)
    for a in range(0, by.shape[0], chunk):
        bits = ((by[a:a + chunk].unsqueeze(-1) >> shifts) & 1).reshape(by[a:a + chunk].shape[0], -1)[:, :n_sym * bps]
        if perm is not None:
            bits = bits[:, perm]
        b = bits.reshape(-1, n_sym, 2, m).to(torch.int64)
        words = (b * wt).sum(dim=-1)
        out[a:a + chunk] = torch.complex(lev_of_word[words[..., 0]], lev_of_word[words[..., 1]])


def main():
    import torch
    assert torch.cuda.is_available() and api.device_count() >= 1, "time_qam.py measures on the GPU"
    dev = torch.device("cuda:0")
    timer = api.Timer()

    def lib_window(run, reps):
        timer.start()
        for _ in range(reps):
            run()
        timer.stop()
        return timer.elapsed_ms() / reps

    def torch_window(run, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def ptr(t):
        return t.data_ptr()

    print(f"# windows of {WINDOW} calls, median of {ROUNDS}; rows / {ROWS_DIV}; torch {torch.__version__}; frac of {CEILING / 1e12:.2f} TB/s")
    print(f"{'N':>5s} {'rows':>6s} {'n_sym':>6s} {'M':>4s} {'dir':>6s} {'csi':>4s} {'perm':>5s} {'ms':>8s} {'GB':>7s} {'frac':>6s} {'torch ms':>9s} {'torch/blk':>9s} {'diff':>8s}")
    rng = np.random.default_rng(synth.SEED)
    for N, Ns, rows in SHAPES:
        rows = max(1, rows // ROWS_DIV)
        idx = data_bins(N)
        Nd, n_sym = idx.size, Ns * idx.size
        csi_idx_t = torch.from_numpy(np.tile(idx.astype(np.int64), Ns)).to(dev)
        csi = torch.view_as_complex(torch.from_numpy(((0.2 + rng.random((rows, N, 1))) * np.exp(2j * np.pi * rng.random((rows, N, 1))))
                                                     .astype(np.complex64).view(np.float32)).to(dev).reshape(rows, N, 2))
        for order in ORDERS:
            bps = {16: 4, 64: 6, 256: 8}[order]
            B = n_sym * bps
            nbytes = (B + 7) // 8
            lev = torch.from_numpy(synth.qam_levels(order, 1.0)).to(dev)
            _, wb = synth.qam_axis_words(bps // 2)
            wbits = torch.from_numpy(wb).to(dev)
            pts, _ = synth.qam_points(order, 1.0)
            z_host = (pts[rng.integers(0, order, size=(rows, n_sym))] + 0.05 * (rng.standard_normal((rows, n_sym)) + 1j * rng.standard_normal((rows, n_sym))))
            z = torch.view_as_complex(torch.from_numpy(z_host.astype(np.complex64).view(np.float32)).to(dev).reshape(rows, n_sym, 2))
            del z_host
            by = torch.from_numpy(rng.integers(0, 256, size=(rows, nbytes), dtype=np.uint8)).to(dev)
            soft, soft_t = (torch.empty((rows, B), dtype=torch.float32, device=dev) for _ in range(2))
            sym, sym_t = (torch.empty((rows, n_sym), dtype=torch.complex64, device=dev) for _ in range(2))
            chunk_d = max(1, (1 << 27) // (n_sym * (1 << (bps // 2))))
            chunk_m = max(1, (1 << 25) // B)
            for with_perm in (False, True):
                perm = rng.permutation(B).astype(np.uint32) if with_perm else None
                perm_t = None if perm is None else torch.from_numpy(perm.astype(np.int64)).to(dev)
                for direction, with_csi in (("map", False), ("demap", False), ("demap", True)):
                    h = api.Qam(order, n_sym, 1.0, 2.0, perm, idx if with_csi else None, N if with_csi else 0)
                    if direction == "demap":
                        block = lambda: h.demap_stream(ptr(z), rows, ptr(soft), ptr(csi) if with_csi else None)
                        tform = lambda: torch_demap(torch, z, lev, wbits, 2.0, csi if with_csi else None, csi_idx_t, perm_t, soft_t, chunk_d)
                        nbytes_moved = rows * (n_sym * (8 + 4 * bps + (4 * bps if with_perm else 0)) + (8 * N if with_csi else 0))
                    else:
                        block = lambda: h.map_stream(ptr(by), rows, ptr(sym))
                        tform = lambda: torch_map(torch, by, lev, bps, perm_t, n_sym, sym_t, chunk_m)
                        nbytes_moved = rows * (nbytes + n_sym * (8 + (4 * bps if with_perm else 0)))
                    block()
                    tform()
                    torch.cuda.synchronize()
                    api.sync()
                    k = min(rows, 8)
                    if direction == "demap":
                        diff = float((soft[:k] - soft_t[:k]).abs().max() / soft_t[:k].abs().max())
                        assert diff <= 1e-5, (N, order, direction, with_csi, with_perm, diff)
                    else:
                        diff = float((torch.view_as_real(sym[:k]) != torch.view_as_real(sym_t[:k])).sum())
                        assert diff == 0, (N, order, direction, with_perm, diff)
                    lib_window(block, 3)
                    torch_window(tform, 1)
                    tb, tt = [], []
                    for _ in range(ROUNDS):
                        tb.append(lib_window(block, WINDOW))
                        tt.append(torch_window(tform, 1))
                    ms, tms = float(np.median(tb)), float(np.median(tt))
                    print(f"{N:>5d} {rows:>6d} {n_sym:>6d} {order:>4d} {direction:>6s} {'yes' if with_csi else 'no':>4s} {'yes' if with_perm else 'no':>5s} "
                          f"{ms:8.3f} {nbytes_moved / 1e9:7.3f} {nbytes_moved / (ms * 1e-3) / CEILING:6.3f} {tms:9.3f} {tms / ms:9.2f} {diff:8.1e}", flush=True)
                    h.close()
            del z, by, soft, soft_t, sym, sym_t
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
