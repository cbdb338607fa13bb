"""Rows and parameter sets the occupancy detector's host and GPU tests share (tests/test_occ_host.py, tests/test_gpu_occ.py):
random rows, and constructed rows of which each hits one branch of the law (include/sfe_dsp.h, sfe_dsp_occ_*), with what
the law must make of it.  Plain numpy; nothing here calls the library."""
import numpy as np

DEFAULTS = dict(rank=0, factor=2.0, min_level=0.0, gap=0, min_width=1, max_emissions=16, shift=False)
# the two parameter sets of the random rows; rank is a fraction of N
SETS = [dict(rank=0.25, factor=3.0, min_level=0.0, gap=2, min_width=1, max_emissions=16, shift=True),
        dict(rank=0.5, factor=1.5, min_level=0.3, gap=0, min_width=2, max_emissions=5, shift=False)]


def params(N, **kw):
    p = dict(DEFAULTS, **kw)
    if isinstance(p["rank"], float):
        p["rank"] = int(p["rank"] * N)
    if N % 2:
        p["shift"] = False
    return p


def random_rows(N, R, seed):
    """Spectrum-like rows: exponential noise around 1, a few raised bands of random place and width (some across the row's
    ends), and every fourth row centred on zero so that negative values take part in the order."""
    rng = np.random.default_rng(seed)
    x = rng.exponential(1.0, (R, N))
    for i in range(R):
        for _ in range(int(rng.integers(0, 6))):
            c, w = int(rng.integers(0, N)), int(rng.integers(1, max(2, N // 6)))
            x[i, np.arange(c, c + w) % N] *= rng.uniform(4.0, 60.0)
        if i % 4 == 3:
            x[i] -= 1.0
    return x.astype(np.float32)


def _row(N, low=1.0):
    return np.full(N, low, np.float32)


def _runs(rec, n):
    return [(int(r["lo"]), int(r["hi"])) for r in rec[:n]]


def constructed():
    """[(name, rows (R, N) float32, params, check)]: check(info, rec, mask) asserts what the law must give for row 0 (and
    the others where it says so); info (R,), rec (R, E), mask (R, N) as api.occ_plan returns them."""
    cases = []

    def add(name, rows, check, **kw):
        rows = np.atleast_2d(np.asarray(rows, np.float32))
        cases.append((name, rows, params(rows.shape[1], **kw), check))

    # all equal: factor >= 1 occupies nothing, factor < 1 everything -- one emission over every tile
    def nothing(info, rec, mask):
        assert info["count"][0] == 0 and info["status"][0] == 0 and not mask.any() and not rec.view(np.uint8).any()
        assert info["floor"][0] == np.float32(0.75) and info["thr"][0] == np.float32(0.75)
    add("equal, factor 1", _row(1000, 0.75), nothing, factor=1.0, rank=500)

    for N in (16, 250, 4096):
        def whole(info, rec, mask, N=N):
            assert info["count"][0] == 1 and _runs(rec[0], 1) == [(0, N - 1)] and mask.all()
            assert rec[0, 0]["peak"] == 0 and rec[0, 0]["peak_val"] == np.float32(0.75)
            assert abs(float(rec[0, 0]["sum"]) - 0.75 * N) < 1e-3 * N
            assert abs(float(rec[0, 0]["moment"]) - 0.75 * N * (N - 1) / 2) < 1e-3 * N * N
        add("equal, factor 0.5, N %d" % N, _row(N, 0.75), whole, factor=0.5, rank=N // 2)

    # alternating high and low: N/2 emissions of width 1 at gap 0 (more than E), one emission at gap 1
    alt = _row(256)
    alt[1::2] = 9.0

    def many(info, rec, mask):
        assert info["count"][0] == 128 and info["status"][0] == 2
        assert _runs(rec[0], 16) == [(p, p) for p in range(1, 33, 2)]
        assert np.array_equal(mask[0], (np.arange(256) % 2).astype(np.uint8))         # the mask holds all of them
    add("alternating, gap 0", alt, many)

    def one(info, rec, mask):
        assert info["count"][0] == 1 and info["status"][0] == 0 and _runs(rec[0], 1) == [(1, 255)]
        assert not rec[0, 1:].view(np.uint8).any() and mask[0, 1:].all() and mask[0, 0] == 0
    add("alternating, gap 1", alt, one, gap=1)

    # gaps of exactly `gap` and of gap + 1
    g = _row(250)
    g[[10, 14, 19]] = 5.0

    def gaps(info, rec, mask):
        assert info["count"][0] == 2 and _runs(rec[0], 2) == [(10, 14), (19, 19)]
        assert rec[0, 0]["sum"] == np.float32(13.0) and rec[0, 0]["moment"] == np.float32(1 + 2 + 3 + 4 * 5)
    add("gaps of gap and gap + 1", g, gaps, gap=3)

    # runs of min_width - 1 and of min_width
    m = _row(250)
    m[20:23] = 5.0
    m[30:34] = 5.0

    def widths(info, rec, mask):
        assert info["count"][0] == 1 and _runs(rec[0], 1) == [(30, 33)] and mask[0].sum() == 4
    add("runs of min_width - 1 and min_width", m, widths, min_width=4)

    # runs that begin or end at p = 0, N - 1, and at 15 or 0 (mod 16)
    e = _row(1024)
    spans = [(0, 0), (12, 15), (32, 40), (63, 64), (79, 95), (320, 335), (511, 512), (1008, 1023)]
    for a, b in spans:
        e[a:b + 1] = 3.0 + np.arange(b - a + 1, dtype=np.float32) % 5

    def edges(info, rec, mask):
        assert info["count"][0] == len(spans) and _runs(rec[0], len(spans)) == spans
    add("runs at the row's and the tiles' edges", e, edges)
    e2 = _row(1024)
    e2[0:17] = 4.0
    e2[1023] = 4.0

    def ends(info, rec, mask):
        assert _runs(rec[0], info["count"][0]) == [(0, 16), (1023, 1023)]
    add("runs at both ends", e2, ends)

    # eight runs inside one tile
    t = _row(256)
    t[32:48:2] = 7.0 + np.arange(8, dtype=np.float32)

    def eight(info, rec, mask):
        assert info["count"][0] == 8 and _runs(rec[0], 8) == [(p, p) for p in range(32, 48, 2)]
        assert np.array_equal(rec[0, :8]["sum"], 7.0 + np.arange(8, dtype=np.float32)) and not rec[0, :8]["moment"].any()
    add("eight runs in one tile", t, eight)

    # equal maxima: the smallest position wins, within a tile and across tiles and waves' lanes
    q = _row(1024)
    q[100:400] = 2.5
    q[[130, 131, 300, 399]] = 8.0
    q[500:520] = 3.0
    q[[507, 519]] = 4.0

    def maxima(info, rec, mask):
        assert _runs(rec[0], info["count"][0]) == [(100, 399), (500, 519)]
        assert list(rec[0, :2]["peak"]) == [130, 507] and list(rec[0, :2]["peak_val"]) == [8.0, 4.0]
    add("equal maxima", q, maxima)

    # many values tied at the rank; the floor is theirs
    ty = _row(250, 2.0)
    ty[:40] = 1.0
    ty[200:210] = 9.0

    def tied(info, rec, mask):
        assert info["floor"][0] == np.float32(2.0) and info["thr"][0] == np.float32(4.0) and _runs(rec[0], info["count"][0]) == [(200, 209)]
    add("ties at the rank", ty, tied, rank=125)

    # negative values, and -0 against +0 at the rank: of N values, 3 negative, then 2 of -0, then 3 of +0
    z = _row(64, 1.0)
    z[:8] = [-3.0, -1.5, -1e-39, -0.0, -0.0, 0.0, 0.0, 0.0]
    z = z[::-1].copy()
    denormal = int(np.array([-1e-39], np.float32).view(np.uint32)[0])
    for rank, bits in ((0, 0xC0400000), (2, denormal), (3, 0x80000000), (4, 0x80000000), (5, 0), (7, 0), (8, 0x3F800000)):
        def signed(info, rec, mask, bits=bits):
            assert info[0:1]["floor"].view(np.uint32)[0] == bits, hex(info[0:1]["floor"].view(np.uint32)[0])
        add("negatives and zeros, rank %d" % rank, z, signed, rank=rank, min_level=-5.0)

    def thr_zero(info, rec, mask):       # factor * (-0) = -0 against min_level +0: the threshold is +0, and nothing at 0 is above it
        assert info[0:1]["thr"].view(np.uint32)[0] == 0 and info["count"][0] == 1 and _runs(rec[0], 1) == [(0, 55)]
    add("-0 against min_level +0", z, thr_zero, rank=3, min_level=0.0)

    def thr_mzero(info, rec, mask):      # factor * (+0) = +0 against min_level -0
        assert info[0:1]["thr"].view(np.uint32)[0] == 0 and info["count"][0] == 1
    add("+0 against min_level -0", z, thr_mzero, rank=6, min_level=-0.0)

    # a NaN, a +inf or a -inf anywhere in the row
    bad = np.stack([_row(250) for _ in range(5)])
    bad[:, 100:110] = 6.0
    bad[0, 0] = np.nan
    bad[1, 249] = np.inf
    bad[2, 128] = -np.inf
    bad[3, 64:66] = np.float32(np.nan), -np.float32(np.nan)

    def nonfinite(info, rec, mask):
        assert list(info["status"]) == [1, 1, 1, 1, 0] and list(info["count"]) == [0, 0, 0, 0, 1]
        assert (info[:4]["floor"].view(np.uint32) == 0x7FC00000).all() and (info[:4]["thr"].view(np.uint32) == 0x7FC00000).all()
        assert not rec[:4].view(np.uint8).any() and not mask[:4].any() and mask[4].sum() == 10
    add("non-finite rows", bad, nonfinite)

    # shift: an emission across DC is one run, in signed bins; the mask stays in the row's own numbering
    for N in (16, 1024):
        d = _row(N)
        d[[N - 2, N - 1, 0, 1]] = [4.0, 5.0, 9.0, 3.0]
        d[N // 2 - 1] = 6.0                         # the last scan position
        d[N // 2] = 7.0                             # the first: the ends of the scan do not join

        def dc(info, rec, mask, N=N):
            assert info["count"][0] == 3 and _runs(rec[0], 3) == [(-N // 2, -N // 2), (-2, 1), (N // 2 - 1, N // 2 - 1)]
            assert rec[0, 1]["peak"] == 0 and rec[0, 1]["peak_val"] == 9.0 and rec[0, 1]["sum"] == 21.0
            assert rec[0, 1]["moment"] == np.float32(5 + 2 * 9 + 3 * 3)
            assert sorted(np.flatnonzero(mask[0])) == sorted([N - 2, N - 1, 0, 1, N // 2 - 1, N // 2])
        add("across DC with shift, N %d" % N, d, dc, shift=True)
    return cases
