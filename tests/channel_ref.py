"""numpy mirror of ldpc_hip_channel_batch (include/ldpc_amd.h states the arithmetic) on top of philox_ref.py: the ASK level
table, the Gray mapping, the max-log demapper, the BSC rule, the conversions to the element types and the quantizer.
sigma2, sigma and delta come from Python's math module — the libm the host code uses — not from numpy.  A `code` is a
gf2_ref.Gf2Code (nc, nct, bit_pos, puncture, shorten)."""
import math

import numpy as np

import philox_ref

SHORTEN_AWGN = 99999.9


def awgn_params(x):
    sigma2 = math.pow(10, -x / 10)
    return sigma2, math.sqrt(sigma2)


def bsc_delta(x):
    return math.log((1 - x) / x)


def levels(m):
    """level[j] = (M - 1 - 2 j) c, c = 1 / sqrt((M^2 - 1) / 3): 2^m-ASK of unit mean energy, binary64."""
    M = 1 << m
    c = 1.0 / math.sqrt(float(M * M - 1) / 3.0)
    return np.asarray([float(M - 1 - 2 * j) * c for j in range(M)], np.float64)


def gray(j):
    return j ^ (j >> 1)


def gray_inverse(g):
    """j with j ^ (j >> 1) == g (labels of up to 4 bits)."""
    g = np.asarray(g)
    return g ^ (g >> 1) ^ (g >> 2) ^ (g >> 3)


def symbols(m, nct):
    return -(-nct // m)


def tx_bits(code, codeword, n):
    """[n, nct] the bits at the transmitted positions (a non-zero byte is 1; None = all zero)."""
    if codeword is None:
        return np.zeros((n, code.nct), np.int64)
    return (np.asarray(codeword)[:, code.bit_pos] != 0).astype(np.int64)


def labels(m, bits):
    """[n, S] the symbols' labels: the m bits of a symbol, the first most significant, padding bits 0."""
    n, nct = bits.shape
    S = symbols(m, nct)
    padded = np.zeros((n, S * m), np.int64)
    padded[:, :nct] = bits
    g = np.zeros((n, S), np.int64)
    for k in range(m):
        g = (g << 1) | padded[:, k::m]
    return g


def awgn_transmit(code, m, codeword, n):
    """[n, S] the levels sent (m = 1: 1 - 2 bit)."""
    bits = tx_bits(code, codeword, n)
    if m == 1:
        return (1 - 2 * bits).astype(np.float64)
    return levels(m)[gray_inverse(labels(m, bits))]


def awgn_received(code, m, x, seed, frames, codeword):
    """The mirror's received values [n, S] (the normals evaluated in binary64 from the device's binary32 arguments) and the
    radius of each one's Box-Muller pair."""
    _, sigma = awgn_params(x)
    S = symbols(m, code.nct)
    normal, radius = philox_ref.awgn_normals(seed, frames, S)
    return normal * sigma + awgn_transmit(code, m, codeword, len(frames)), radius


def demap(m, y, sigma2):
    """[n, S] received -> [n, S, m] LLRs; m = 1: (2 y) / sigma2, else max-log over the level table."""
    y = np.asarray(y, np.float64)
    if m == 1:
        return ((2 * y) / sigma2)[..., None]
    return demap_max_log(m, y, sigma2)


def demap_max_log(m, y, sigma2):
    lv = levels(m)
    e = y[..., None] - lv
    d = e * e
    lab = gray(np.arange(1 << m))
    out = np.empty(y.shape + (m,), np.float64)
    for k in range(m):
        bit = (lab >> (m - 1 - k)) & 1
        d0 = np.min(d[..., bit == 0], axis=-1)
        d1 = np.min(d[..., bit == 1], axis=-1)
        out[..., k] = (d1 - d0) / (2 * sigma2)
    return out


def scatter(code, per_bit, shorten_value):
    """[n, >= nct] values of the transmitted bits -> [n, nc] in column order; punctured and unconnected columns +0.0,
    shortened columns shorten_value."""
    n = per_bit.shape[0]
    out = np.zeros((n, code.nc), np.float64)
    out[:, code.shorten] = shorten_value
    out[:, code.bit_pos] = per_bit[:, :code.nct]
    return out


def awgn_llr(code, m, x, received):
    """The LLRs [n, nc] (binary64) the call returns for its own received values."""
    sigma2, _ = awgn_params(x)
    per_bit = demap(m, received, sigma2).reshape(received.shape[0], -1)
    return scatter(code, per_bit, SHORTEN_AWGN)


def bsc(code, x, seed, frames, codeword):
    """(received [n, nct], llr [n, nc]) of the BSC: exact."""
    bits = tx_bits(code, codeword, len(frames))
    ybit = bits ^ philox_ref.draws(seed, frames, code.nct, x).astype(np.int64)
    received = (1 - 2 * ybit).astype(np.float64)
    delta = bsc_delta(x)
    return received, scatter(code, delta * received, delta)


def quantize(llr, q_bits, step):
    """clamp(rint(fl(L * inv)), -Qmax, +Qmax), inv = fl(1 / step), the clamp in binary64, a NaN gives 0 -> int8."""
    inv = 1.0 / step
    qmax = (1 << (q_bits - 1)) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(llr, np.float64) * inv)
    r = np.where(np.isnan(r), 0.0, np.clip(r, -qmax, qmax))
    return r.astype(np.int8)


def convert(llr, kind, q_bits=0, step=1.0):
    """The binary64 LLRs in the element type `kind` of the call."""
    with np.errstate(over="ignore"):
        if kind == "float64":
            return np.asarray(llr, np.float64)
        if kind == "float32":
            return llr.astype(np.float32)
        if kind == "float16":
            return llr.astype(np.float32).astype(np.float16)
    return quantize(llr, q_bits, step)


def raw(a):
    """The bit patterns of an array, for comparisons that tell -0.0 from +0.0 and see every NaN."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
