"""What the frame check's tests share (sfe_dsp_crc_*): the catalogue rows with their published check values and residues,
the two published scrambler sequences, the payload lengths, and seeded rows.  Nothing here runs the code under test."""
import numpy as np

CHECK_MESSAGE = b"123456789"
# name: (width, poly, init, reflect, xorout), the CRC of CHECK_MESSAGE
CATALOGUE = {
    "CRC-32/ISO-HDLC": ((32, 0x04C11DB7, 0xFFFFFFFF, 1, 0xFFFFFFFF), 0xCBF43926),
    "CRC-32/ISCSI": ((32, 0x1EDC6F41, 0xFFFFFFFF, 1, 0xFFFFFFFF), 0xE3069283),
    "CRC-32/MPEG-2": ((32, 0x04C11DB7, 0xFFFFFFFF, 0, 0), 0x0376E6E7),
    "CRC-32/BZIP2": ((32, 0x04C11DB7, 0xFFFFFFFF, 0, 0xFFFFFFFF), 0xFC891918),
    "CRC-24/OPENPGP": ((24, 0x864CFB, 0xB704CE, 0, 0), 0x21CF02),
    "CRC-24/LTE-A": ((24, 0x864CFB, 0, 0, 0), 0xCDE703),
    "CRC-16/XMODEM": ((16, 0x1021, 0, 0, 0), 0x31C3),
    "CRC-16/IBM-3740": ((16, 0x1021, 0xFFFF, 0, 0), 0x29B1),
    "CRC-16/KERMIT": ((16, 0x1021, 0, 1, 0), 0x2189),
    "CRC-16/ARC": ((16, 0x8005, 0, 1, 0), 0xBB3D),
    "CRC-16/IBM-SDLC": ((16, 0x1021, 0xFFFF, 1, 0xFFFF), 0x906E),
    "CRC-8/SMBUS": ((8, 0x07, 0, 0, 0), 0xF4),
    "CRC-8/MAXIM-DOW": ((8, 0x31, 0, 1, 0), 0xA1),
}
NAMES = sorted(CATALOGUE)
# the CRC of payload || tail with xorout taken as 0; 0 for every row whose xorout is 0
RESIDUE = {"CRC-32/ISO-HDLC": 0xDEBB20E3, "CRC-32/ISCSI": 0xB798B438, "CRC-32/BZIP2": 0xC704DD7B, "CRC-16/IBM-SDLC": 0xF0B8}

# (m, taps, seed): the CCSDS randomiser's first bytes; the IEEE 802.11 sequence from bit 7 of the bytes on, period 127
PN_CCSDS = (8, 0xA9, 0xFF)
PN_CCSDS_BYTES = bytes.fromhex("ff480ec09a0d70bc8e2c93ada7b746ce")
PN_80211 = (7, 0x09, 0x7F)
PN_80211_BITS = "00001110" "11110010" "11001001" "00000010" "00100110"
PN_80211_PERIOD = 127
PN_LONG = (32, 0x00400007, 0x12345678)          # a degree-32 register, for the width of the state

HOST_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 4099)


def rows(n_frames, n_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n_frames, n_bytes), dtype=np.uint8)


def model(name):
    return CATALOGUE[name][0]
