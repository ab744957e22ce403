# coding=utf-8
"""The neighbour sampler's draws restated in plain Python integers (csrc/tfgx_sample_rows.h): the generator, the lane / wave
split, both per-row bodies and the count rules.  Positions are relative to the row's first CSR entry, in output order; the
caller maps them to (col, w), which the kernels copy and never compute."""
import math

_M64 = (1 << 64) - 1
LONG_ROW, FLOYD_MAX, WAVE = 64, 32, 64


def draw_u32(seed, row, i):
    z = (seed + 0x9E3779B97F4A7C15 * ((row * 0x100000001B3 + i + 1) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) >> 32


def draw_below(seed, row, i, n):
    return (draw_u32(seed, row, i) * n) >> 32


def row_is_long(d, m):
    return (d > LONG_ROW and m > FLOYD_MAX) or m > LONG_ROW


def draws(d, k=None, ratio=None, padding=False):
    """How many neighbours a row of degree d draws."""
    if k is None and ratio is None:
        return d
    if ratio is not None:
        return int(math.ceil(float(d) * float(ratio)))
    if padding:
        return int(k) if d > 0 else 0
    return min(d, int(k))


def _selection(seed, row, lo, hi, m):
    """Algorithm S: m of the positions [lo, hi), in increasing order."""
    out = []
    for j in range(lo, hi):
        if len(out) >= m:
            break
        if draw_below(seed, row, j, hi - j) < m - len(out):
            out.append(j)
    return out


def _lane(seed, row, d, m):
    if m > FLOYD_MAX:
        return _selection(seed, row, 0, d, m)
    chosen = []                                                     # Floyd
    for j in range(d - m, d):
        t = draw_below(seed, row, j - (d - m), j + 1)
        chosen.append(j if t in chosen else t)
    return chosen


def _wave(seed, row, d, m):
    out = [None] * m
    U = draw_below(seed, row, 0xFFFFFFFF, d)
    for lane in range(WAVE):
        b0, b1 = d * lane // WAVE, d * (lane + 1) // WAVE
        o0 = (m * b0 + U) // d
        ml = (m * b1 + U) // d - o0
        for t, j in enumerate(_selection(seed, row, b0, b1, ml)):
            out[o0 + t] = j
    return out


def sample_row(seed, row, d, m, padding=False):
    """The m positions of [0, d) that the row keyed `row` draws (d > 0, m > 0), in output order."""
    if m >= d and not (padding and m > d):
        return list(range(d))
    if m > d:
        return [draw_below(seed, row, i, d) for i in range(m)]
    return _wave(seed, row, d, m) if row_is_long(d, m) else _lane(seed, row, d, m)


def sample_graph(row_ptr, seed, k=None, ratio=None, padding=False):
    """(rows, CSR positions) of the whole-graph sample: row r is keyed by r."""
    rows, pos = [], []
    for r in range(len(row_ptr) - 1):
        s, d = int(row_ptr[r]), int(row_ptr[r + 1] - row_ptr[r])
        m = draws(d, k, ratio, padding)
        if d <= 0 or m <= 0:
            continue
        p = sample_row(seed, r, d, m, padding)
        rows += [r] * len(p)
        pos += [s + t for t in p]
    return rows, pos
