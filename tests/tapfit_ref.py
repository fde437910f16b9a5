"""The tap fit (include/gdg.h, TAPFIT) restated in numpy: the V = K T + 1 shifted rows of a block, their Gram exactly (int64 for integer rows,
math.fsum otherwise), the packed record, and the planner -- the unpivoted Cholesky solve in virtual-row order.  No device, no library."""
import math

import numpy as np

EPS = 2.0 ** -52


def fit_doubles(terms, taps):
    V = terms * taps + 1
    return V * (V + 1) // 2


def list_doubles(fits):
    """fits = [(target, [ports], taps), ...] -> D"""
    return sum(fit_doubles(len(ports), T) for _, ports, T in fits)


def shifted_rows(rows, target, ports, taps, first=0, length=None):
    """the virtual rows of one block [first, first + length): row j T + a is x[p_j][i - a], the last one x[t][i], i = first + T - 1 + n,
    n = 0 .. length - T -> [V, max(length - T + 1, 0)]; nothing outside the block is read"""
    rows = np.asarray(rows)
    length = rows.shape[1] - first if length is None else length
    n = max(length - taps + 1, 0)
    out = np.zeros((len(ports) * taps + 1, n), dtype=rows.dtype)
    if n == 0:
        return out
    blk = rows[:, first:first + length]
    for j, p in enumerate(ports):
        for a in range(taps):
            out[j * taps + a] = blk[p, taps - 1 - a:taps - 1 - a + n]
    out[-1] = blk[target, taps - 1:taps - 1 + n]
    return out


def packed(G):
    return G[np.tril_indices(G.shape[0])].copy()


def record_int(rows, fits, block):
    """integer rows: the exact records [blocks, D] as float64 (every sum must stay below 2^53)"""
    rows = np.asarray(rows, dtype=np.int64)
    samples = rows.shape[1]
    out = []
    for b in range(-(-samples // block)):
        L = min(block, samples - b * block)
        parts = []
        for t, ports, T in fits:
            v = shifted_rows(rows, t, ports, T, b * block, L)
            parts.append(packed(v @ v.T).astype(np.float64))
        out.append(np.concatenate(parts))
    return np.stack(out)


def entry_fsum(v, u, w):
    """the exact inner product of virtual rows u and w, and sum |a b|"""
    p = v[u] * v[w]
    return math.fsum(p), math.fsum(np.abs(p))


def unpack(record, terms, taps):
    """one fit's part of a record -> the full symmetric [V, V] matrix"""
    V = terms * taps + 1
    G = np.zeros((V, V))
    G[np.tril_indices(V)] = record
    return G + np.tril(G, -1).T


def solve(G, ridge=0.0):
    """the planner on one summed [V, V] Gram: (A + ridge mean(diag A) I) h = b by an unpivoted Cholesky in row order -> (h, residual), or
    ("pivot", row) where a pivot is at or below U 2^-52 max(diag A).  Plain float64 in the library's order of operations."""
    U = G.shape[0] - 1
    A, b, Tt = G[:U, :U], G[U, :U], G[U, U]
    shift = ridge * (float(sum(A[j, j] for j in range(U))) / U)
    least = U * EPS * max(max(A[j, j] for j in range(U)), 0.0)
    Lo = np.zeros((U, U))
    for j in range(U):
        d = A[j, j] + shift
        for k in range(j):
            d -= Lo[j, k] * Lo[j, k]
        if not d > least:
            return "pivot", j
        Lo[j, j] = math.sqrt(d)
        for i in range(j + 1, U):
            s = A[i, j]
            for k in range(j):
                s -= Lo[i, k] * Lo[j, k]
            Lo[i, j] = s / Lo[j, j]
    y, h = np.zeros(U), np.zeros(U)
    for j in range(U):
        s = b[j]
        for k in range(j):
            s -= Lo[j, k] * y[k]
        y[j] = s / Lo[j, j]
    for j in range(U - 1, -1, -1):
        s = y[j]
        for k in range(j + 1, U):
            s -= Lo[k, j] * h[k]
        h[j] = s / Lo[j, j]
    hb, hAh = 0.0, 0.0
    for j in range(U):
        hb += h[j] * b[j]
        row = 0.0
        for k in range(U):
            row += A[j, k] * h[k]
        hAh += h[j] * row
    left = Tt - 2.0 * hb + hAh
    return h, (0.0 if Tt == 0.0 else max(left, 0.0) / Tt)


def plan(records, fits, ridge=0.0):
    """records [blocks, D] -> per fit (h [terms, T], residual): the blocks added in block order with plain adds, then solve()"""
    records = np.asarray(records, dtype=np.float64)
    out, off = [], 0
    for _, ports, T in fits:
        E = fit_doubles(len(ports), T)
        total = np.zeros(E)
        for q in range(records.shape[0]):
            total = total + records[q, off:off + E]
        h, res = solve(unpack(total, len(ports), T), ridge)
        out.append((h if isinstance(h, str) else h.reshape(len(ports), T), res))
        off += E
    return out


def lstsq_taps(rows, target, ports, taps, block):
    """numpy.linalg.lstsq on the shifted rows of all blocks -> (h [terms, T], residual share, cond(A)): the independent reference"""
    cols = [shifted_rows(rows, target, ports, taps, b * block, min(block, rows.shape[1] - b * block)) for b in range(-(-rows.shape[1] // block))]
    v = np.concatenate(cols, axis=1)
    X, t = v[:-1].T, v[-1]
    h, _, _, sv = np.linalg.lstsq(X, t, rcond=None)
    r = t - X @ h
    return h.reshape(len(ports), taps), float(r @ r) / float(t @ t), float(sv[0] / sv[-1]) ** 2
