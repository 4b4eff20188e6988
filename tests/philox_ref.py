"""Python restatement of the counter-based noise mode (include/ldpc_amd.h, ldpc_hip_set_noise): Philox4x32-10
and the layout of the AWGN normals, BSC / BEC draws and encoder info bits over (seed, frame, bit).  numpy only."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
TAG_AWGN, TAG_DRAW, TAG_INFO = 0, 1, 2

# Random123's published known answers: (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(c, k):
    """c: four arrays (or ints) of 32-bit counter words, k: two key words -> [..., 4] uint32."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & M32 for x in c)
    k0, k1 = (np.asarray(x, np.uint64) & M32 for x in k)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)  # (products of 32-bit words: exact in 64 bits)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def blocks(seed, tag, frames, blks):
    """Words [len(frames), len(blks), 4] of blocks `blks` of frames `frames` under tag."""
    f = np.asarray(frames, np.uint64).reshape(-1, 1)
    b = np.asarray(blks, np.uint64).reshape(1, -1)
    seed = np.uint64(seed)
    return philox4x32_10((b, f & M32, f >> np.uint64(32), np.uint64(tag)), (seed & M32, seed >> np.uint64(32)))


def box_muller(w):
    """[..., 4] words -> [..., 4] normals, the device's binary32 arguments (u = (w0 + 0.5) / 2^32 and t = w1 / 2^32
    rounded to binary32 as the device rounds them) evaluated in binary64."""
    wf = w.astype(np.float32)
    u = wf[..., 0::2] * np.float32(2.0**-32) + np.float32(2.0**-33)  # (the product is exact: one rounding, as fmaf)
    t = (wf[..., 1::2] * np.float32(2.0**-32)).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    out = np.empty(w.shape, np.float64)
    out[..., 0::2] = r * np.cos(2 * np.pi * t)
    out[..., 1::2] = r * np.sin(2 * np.pi * t)
    return out, np.repeat(r, 2, axis=-1)


def awgn_normals(seed, frames, nct):
    """normals [len(frames), nct] of transmitted bits 0..nct-1, and the radius of each one's pair"""
    n, r = box_muller(blocks(seed, TAG_AWGN, frames, np.arange((nct + 3) // 4)))
    return n.reshape(len(frames), -1)[:, :nct], r.reshape(len(frames), -1)[:, :nct]


def draws(seed, frames, nct, eps):
    """flip / erase decisions [len(frames), nct]: (w + 0.5) / 2^32 < eps (exact in binary64)"""
    w = blocks(seed, TAG_DRAW, frames, np.arange((nct + 3) // 4)).reshape(len(frames), -1)[:, :nct]
    return (w.astype(np.float64) + 0.5) * 2.0**-32 < eps


def info_bits(seed, frames, kc):
    """info words [len(frames), kc]: bit j = bit j % 32 of word (j / 32) % 4 of block j / 128"""
    w = blocks(seed, TAG_INFO, frames, np.arange((kc + 127) // 128)).reshape(len(frames), -1)
    j = np.arange(kc)
    return ((w[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(np.uint8)
