"""The frame check's host plan (sfe_dsp_crc_plan, sfe_dsp_crc_pn_bytes: csrc/crc_law.h compiled for the host, a byte at a time
through a table) against references that share nothing with it: the published check values and residues of the catalogue
(tests/crc_cases.py), zlib.crc32, binascii.crc_hqx, the two published scrambler sequences, and synth.crc_reference /
synth.pn_reference, the bit-serial numpy restatements of the law -- bytes, record and status with array_equal.  Then what
a CRC is for (every single-bit flip and every burst of up to w bits is caught), the upstream convention, the refusals, the
build's bookkeeping, and the law through a stand-alone program built with -fsanitize=address,undefined
(tests/host/test_crc_law.cpp).  No GPU."""
import binascii
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import crc_cases as cc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDLC, XMODEM = cc.model("CRC-32/ISO-HDLC"), cc.model("CRC-16/XMODEM")


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a, build
    build.build_lib()
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def same(got, want, what):
    for name, g, w in zip(("bytes", "record", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def tail_value(tail, reflect):
    return int.from_bytes(bytes(tail), "little" if reflect else "big")


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_plan_gives_the_catalogue_check_value_and_residue(api, name):
    m, want = cc.CATALOGUE[name]
    w, poly, init, reflect, xorout = m
    msg = np.frombuffer(cc.CHECK_MESSAGE, np.uint8)
    frame = api.crc_plan(*m, payload_bytes=9, data=msg)
    assert frame.shape == (1, 9 + w // 8) and frame[0, :9].tobytes() == cc.CHECK_MESSAGE
    assert tail_value(frame[0, 9:], reflect) == want
    by, rec, st = api.crc_plan(*m, payload_bytes=9, data=frame, verify=True)
    assert by.tobytes() == cc.CHECK_MESSAGE and rec.tolist() == [[want, want]] and st.tolist() == [0]
    # the residue: the CRC of payload || tail with xorout taken as 0, for this and for seeded payloads
    for P, seed in ((9, None), (1, 1), (31, 2), (1024, 3)):
        pay = msg[None, :] if seed is None else cc.rows(3, P, seed)
        frames = api.crc_plan(*m, payload_bytes=P, data=pay)
        res = api.crc_plan(w, poly, init, reflect, 0, payload_bytes=P + w // 8, data=frames)[:, P + w // 8:]
        assert [tail_value(r, reflect) for r in res] == [cc.RESIDUE.get(name, 0)] * len(frames), (name, P)


def test_the_plan_equals_zlib_and_crc_hqx(api):
    rng = np.random.default_rng(7)
    for P in (1, 2, 3, 4, 5, 63, 64, 65, 1020, 4099, 65541, 1 << 20):
        pay = cc.rows(2, P, P)
        frames = api.crc_plan(*HDLC, payload_bytes=P, data=pay)
        assert [tail_value(f[P:], 1) for f in frames] == [zlib.crc32(r.tobytes()) for r in pay], P
        rec = api.crc_plan(*HDLC, payload_bytes=P, data=frames, verify=True)[1]
        assert rec[:, 0].tolist() == [zlib.crc32(r.tobytes()) for r in pay]
    for P in (1, 2, 5, 257, 1024, 4099, int(rng.integers(5000, 70000))):
        pay = cc.rows(2, P, P + 1)
        for init in (0, 0xFFFF):
            frames = api.crc_plan(16, 0x1021, init, 0, 0, payload_bytes=P, data=pay)
            assert [tail_value(f[P:], 0) for f in frames] == [binascii.crc_hqx(r.tobytes(), init) for r in pay], (P, init)


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_plan_equals_the_reference(api, name):
    """Every payload length, with and without a scrambler, append and check (clean frames, damaged frames, a status table):
    bytes, record and status."""
    m = cc.model(name)
    for P in cc.HOST_LENGTHS:
        for pn in ((0, 0, 0), cc.PN_CCSDS if P % 2 else cc.PN_LONG):
            shape = (*m, *pn, P)
            pay = cc.rows(5, P, P + len(name))
            frames = api.crc_plan(*shape, data=pay)
            want = synth.crc_reference(*shape, data=pay)
            assert frames.dtype == want.dtype and np.array_equal(frames, want), (name, P, pn)
            assert frames.shape == (5, api.crc_plan(*shape))
            hit = frames.copy()
            hit[1, 0] ^= 0x80
            hit[3, -1] ^= 0x01
            hit[4, P // 2] ^= 0x10
            si = [0, 0, 5, 0, 0]
            same(api.crc_plan(*shape, data=hit, verify=True), synth.crc_reference(*shape, data=hit, verify=True), (name, P, pn))
            got = api.crc_plan(*shape, data=hit, verify=True, status_in=si)
            same(got, synth.crc_reference(*shape, data=hit, verify=True, status_in=si), (name, P, pn, "status_in"))
            assert got[2].tolist() == [0, 1, 2, 1, 1] and np.array_equal(got[0][0], pay[0])


def test_pn_bytes_gives_the_published_sequences(api):
    assert api.pn_bytes(*cc.PN_CCSDS, 16).tobytes() == cc.PN_CCSDS_BYTES
    bits = np.unpackbits(api.pn_bytes(*cc.PN_80211, 40))
    assert "".join(map(str, bits[7:7 + len(cc.PN_80211_BITS)])) == cc.PN_80211_BITS
    assert np.array_equal(bits[:127], bits[127:254]) and not any(np.array_equal(bits[:127], np.roll(bits[:127], k)) for k in range(1, 127))
    for pn, n in ((cc.PN_CCSDS, 700), (cc.PN_80211, 33), (cc.PN_LONG, 4103), ((2, 0x3, 0x1), 9), ((32, 0x80000001, 0xFFFFFFFF), 64)):
        got = api.pn_bytes(*pn, n)
        assert got.dtype == np.uint8 and np.array_equal(got, synth.pn_reference(*pn, n)), pn
    assert api.pn_bytes(*cc.PN_CCSDS, 0).size == 0


def test_scrambling_twice_is_the_identity_and_reed_takes_the_sequence(api):
    P = 1021
    pay = cc.rows(4, P, 5)
    shape = (0, 0, 0, 0, 0, *cc.PN_CCSDS, P)              # a scrambler alone: Fb = P
    assert api.crc_plan(*shape) == P
    once = api.crc_plan(*shape, data=pay)
    assert np.array_equal(once, pay ^ api.pn_bytes(*cc.PN_CCSDS, P)[None, :]) and not np.array_equal(once, pay)
    assert np.array_equal(api.crc_plan(*shape, data=once), pay)
    by, rec, st = api.crc_plan(*shape, data=once, verify=True, status_in=[0, 1, 0, 0])
    assert np.array_equal(by[[0, 2, 3]], pay[[0, 2, 3]]) and not by[1].any() and not rec.any() and st.tolist() == [0, 2, 0, 0]
    code = (0x11d, 1, 1, 40, 8, 3)
    wh = api.pn_bytes(*cc.PN_CCSDS, 120)
    data = cc.rows(2, 96, 6)
    assert np.array_equal(api.reed_plan(*code, whiten=wh, data=data, encode=True), api.reed_plan(*code, data=data, encode=True) ^ wh[None, :])


def test_every_bit_flip_and_every_short_burst_is_caught(api):
    """One 24-byte CRC-16 frame: all 8 Fb single-bit flips, payload and tail, and every burst of 2 .. 16 bits at every
    offset (a burst: its first and last bit flipped, those between as seeded) give status 1; the untouched frame 0."""
    P, w = 22, 16
    shape = (*XMODEM, *cc.PN_80211, P)
    frame = api.crc_plan(*shape, data=cc.rows(1, P, 9))
    Fb = frame.shape[1]
    assert Fb == 24 and api.crc_plan(*shape, data=frame, verify=True)[2].tolist() == [0]
    bits = np.unpackbits(frame[0])
    flips = np.repeat(bits[None, :], 8 * Fb, axis=0) ^ np.eye(8 * Fb, dtype=np.uint8)
    st = api.crc_plan(*shape, data=np.packbits(flips, axis=1), verify=True)[2]
    assert st.shape == (8 * Fb,) and (st == 1).all()
    rng = np.random.default_rng(3)
    bursts = []
    for length in range(2, w + 1):
        for at in range(8 * Fb - length + 1):
            e = np.zeros(8 * Fb, np.uint8)
            e[at] = e[at + length - 1] = 1
            e[at + 1:at + length - 1] = rng.integers(0, 2, size=length - 2)
            bursts.append(bits ^ e)
    st = api.crc_plan(*shape, data=np.packbits(np.array(bursts), axis=1), verify=True)[2]
    assert st.size == sum(8 * Fb - n + 1 for n in range(2, w + 1)) and (st == 1).all()


def test_marked_frames_are_not_read_and_each_output_may_be_null(api, L):
    lib = L.load()
    P = 37
    m = cc.model("CRC-24/OPENPGP")
    shape = (*m, *cc.PN_CCSDS, P)
    Fb = P + 3
    frames = api.crc_plan(*shape, data=cc.rows(6, P, 11))
    frames[4, 2] ^= 4
    by, rec, st = api.crc_plan(*shape, data=frames, verify=True)
    # a marked frame's input is not read: it lies outside the buffer handed in
    si = np.array([0, 0, 0, 0, 0, 7], np.int32)
    short = np.ascontiguousarray(frames[:5])
    b2, r2, s2 = np.full((6, P), 0xA5, np.uint8), np.full((6, 2), 0xA5A5A5A5, np.uint32), np.full(6, -3, np.int32)
    head = (*shape, 1, short.ctypes.data, Fb, si.ctypes.data, 6)
    assert lib.sfe_dsp_crc_plan(*head, b2.ctypes.data, P, r2.ctypes.data, s2.ctypes.data, None) == L.SFE_OK
    assert np.array_equal(b2[:5], by[:5]) and np.array_equal(r2[:5], rec[:5]) and np.array_equal(s2[:5], st[:5]) and st.tolist() == [0, 0, 0, 0, 1, 0]
    assert not b2[5].any() and r2[5].tolist() == [0, 0] and s2[5] == 2
    head = (*shape, 1, frames.ctypes.data, Fb, None, 6)
    b3, r3, s3 = np.zeros_like(by), np.zeros_like(rec), np.zeros_like(st)
    assert lib.sfe_dsp_crc_plan(*head, b3.ctypes.data, P, None, None, None) == L.SFE_OK and np.array_equal(b3, by)
    assert lib.sfe_dsp_crc_plan(*head, None, 0, r3.ctypes.data, None, None) == L.SFE_OK and np.array_equal(r3, rec)
    assert lib.sfe_dsp_crc_plan(*head, None, 0, None, s3.ctypes.data, None) == L.SFE_OK and np.array_equal(s3, st)
    assert lib.sfe_dsp_crc_plan(*head, None, 0, None, None, None) == L.SFE_OK
    f = C.c_int(-1)
    assert lib.sfe_dsp_crc_plan(*shape, 0, None, 0, None, 0, None, 0, None, None, C.byref(f)) == L.SFE_OK and f.value == Fb


def test_refusals_and_their_prefix(api, L):
    lib = L.load()
    order = ("width", "poly", "init", "reflect", "xorout", "pn_m", "pn_taps", "pn_seed", "payload_bytes")
    good = dict(width=16, poly=0x1021, init=0xFFFF, reflect=0, xorout=0, pn_m=7, pn_taps=0x09, pn_seed=0x7F, payload_bytes=24)
    tail = (0, None, 0, None, 0, None, 0, None, None, None)
    assert lib.sfe_dsp_crc_plan(*[good[k] for k in order], *tail) == L.SFE_OK
    bad = [dict(width=12), dict(width=40), dict(width=-8), dict(poly=0x1020), dict(poly=0x11021), dict(init=0x10000), dict(xorout=0x10000),
           dict(width=8, poly=0x107, init=0, xorout=0), dict(reflect=2), dict(pn_m=1), dict(pn_m=33), dict(pn_m=-1), dict(pn_taps=0x08),
           dict(pn_taps=0x89), dict(pn_seed=0), dict(pn_seed=0x80), dict(payload_bytes=0), dict(payload_bytes=(1 << 20) + 1),
           dict(width=0, pn_m=0)]
    h = C.c_void_p(1)
    for change in bad:
        a = [dict(good, **change)[k] for k in order]
        assert lib.sfe_dsp_crc_plan(*a, *tail) == L.SFE_EINVAL, change
        assert lib.sfe_dsp_last_error().startswith(b"crc: "), lib.sfe_dsp_last_error()
        # create refuses them before it looks for a device: SFE_EINVAL on a machine with no GPU too
        assert lib.sfe_dsp_crc_create(*a, 0, C.byref(h)) == L.SFE_EINVAL and h.value is None, change
        assert lib.sfe_dsp_last_error().startswith(b"crc: ")
        h.value = 1
    a = [good[k] for k in order]
    assert lib.sfe_dsp_crc_plan(*a, 2, *tail[1:]) == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"crc: ")      # check = 2
    assert lib.sfe_dsp_crc_plan(*[dict(good, payload_bytes=1 << 20)[k] for k in order], *tail) == L.SFE_OK
    P, Fb = 24, 26
    buf, res = np.zeros(4 * Fb, np.uint8), np.zeros(4 * Fb, np.uint8)
    for chk, istride, ostride in ((1, Fb - 1, P), (1, Fb, P - 1), (0, P - 1, Fb), (0, P, Fb - 1)):
        assert lib.sfe_dsp_crc_plan(*a, chk, buf.ctypes.data, istride, None, 2, res.ctypes.data, ostride, None, None, None) == L.SFE_ERANGE
        assert lib.sfe_dsp_last_error().startswith(b"crc: ")
    out = np.zeros(4, np.uint8)
    for m, taps, seed in ((0, 1, 1), (1, 1, 1), (33, 1, 1), (8, 0xA8, 1), (8, 0x1A9, 1), (8, 0xA9, 0), (8, 0xA9, 0x100)):
        assert lib.sfe_dsp_crc_pn_bytes(m, taps, seed, 4, out.ctypes.data) == L.SFE_EINVAL, (m, taps, seed)
        assert lib.sfe_dsp_last_error().startswith(b"crc: ")
    assert lib.sfe_dsp_crc_pn_bytes(8, 0xA9, 0xFF, 4, None) == L.SFE_EINVAL
    with pytest.raises(api.SfeError):
        api.crc_plan(16, 0x1020, 0, 0, 0, payload_bytes=4)
    with pytest.raises(ValueError):
        api.crc_plan(*XMODEM, payload_bytes=4, data=np.zeros((2, 6), np.uint8), verify=True, status_in=[0])
    if not os.path.exists("/dev/kfd"):
        with pytest.raises(api.SfeError) as e:
            api.Crc(*XMODEM, payload_bytes=24)
        assert e.value.code == L.SFE_ENODEV
    k = C.c_size_t(5)
    assert lib.sfe_dsp_crc_check_stream(None, None, 26, None, 1, None, 24, None, None, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"crc_check_stream: ")
    k.value = 5
    assert lib.sfe_dsp_crc_append_stream(None, None, 24, 1, None, 26, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"crc_append_stream: ")
    assert lib.sfe_dsp_crc_destroy(None) == L.SFE_OK


def test_the_kernels_are_registered_and_touch_no_scratch(api):
    import json
    import re
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "crc.hip.resources.json")))
    assert len(res) == 4 and all("crc_kernel<" in k for k in res)
    assert sum("crc_kernel<64, 4," in k for k in res) == 2 and sum("crc_kernel<1024, 1," in k for k in res) == 2
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] <= 64 and r["Occupancy"] >= 8, (k, r)
    assert "crc.hip" in build.EXACT_SOURCES and "api_crc.hip" in build.HOST_SOURCES and build.SCRATCH_FREE["crc.hip"]
    assert build.KERNEL_FILES["crc"] == ("crc.hip", "crc.h", "crc_law.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bcrc\.hip\b", cm)


def test_the_law_under_the_sanitizers(tmp_path):
    """tests/host/test_crc_law.cpp, built with the host compiler and -fsanitize=address,undefined: the serial law, the plan's
    byte table and a host restatement of the kernels' fold over 64 and 1024 lanes (with the constants a handle makes at
    create) agree over the catalogue and over seeded models and lengths; whole frames go through heap blocks of exactly
    the contract's sizes."""
    exe = str(tmp_path / "crc_law")
    r = subprocess.run(["g++", "-O1", "-Wall", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_crc_law.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "crc law ok: " in r.stdout, r.stdout + r.stderr
