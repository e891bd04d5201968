"""A plain NumPy model of ONE launch of the tile kernels, and the data the launch-level tests feed them.

Written from the comments of csrc/gprn_internal.h (TileTask), csrc/gemm_tile.hip and csrc/tile_mma.h: what a launch is
documented to do to its buffers, not how its loops do it.  A task is the 8-tuple the C ABI takes (gprn_test_tile_launch):
(c_off, a_off, b_off, klen, c_buf, a_buf, b_buf, modes).  Buffers are (nbatch, nbuf, ld, ld) float64 arrays.

Everything here is exact on the data it is used with: small integers (every product and partial sum representable, so
any summation order gives the same bits) or dyadic fractions (sym_data).
"""
import numpy as np

TILE, KC = 128, 16
BUF_B, BUF_X, BUF_K, BUF_KLINV = 0, 1, 2, 3
CM_SET, CM_SUB, CM_SETNEG = 0, 1, 2
TS_128x128, TS_64x64, TS_64x128, TS_128x64, TS_64x128_BTRI, TS_128x64_ATRI = range(6)
TG_PANEL, TG_INNER, TG_NEXT, TG_BULK, TG_MISC, TG_AHEAD, TG_COV = range(7)
LOWER, FIRST_TOUCH = 16, 32                                  # modes bits 4 and 5

# every (shape, tag) launch_tiles has a kernel for
PAIRS = [(TS_64x128_BTRI, TG_PANEL), (TS_128x64_ATRI, TG_PANEL),
         (TS_64x64, TG_INNER), (TS_128x128, TG_INNER), (TS_64x64, TG_NEXT), (TS_128x128, TG_NEXT),
         (TS_64x64, TG_BULK), (TS_128x128, TG_BULK), (TS_64x64, TG_AHEAD), (TS_128x128, TG_AHEAD),
         (TS_128x128, TG_MISC), (TS_64x64, TG_MISC), (TS_64x128, TG_MISC), (TS_128x64, TG_MISC),
         (TS_64x64, TG_COV)]
SHAPE_NAMES = ['128x128', '64x64', '64x128', '128x64', '64x128_BTRI', '128x64_ATRI']
TAG_NAMES = ['PANEL', 'INNER', 'NEXT', 'BULK', 'MISC', 'AHEAD', 'COV']


def pair_id(pair):
    return '%s-%s' % (SHAPE_NAMES[pair[0]], TAG_NAMES[pair[1]])


def can_lower(shape, tag):
    """bit 4 restricts the 64 x 64 form of these families to the lower 16 x 16 blocks"""
    return shape == TS_64x64 and tag in (TG_INNER, TG_NEXT, TG_BULK, TG_AHEAD, TG_COV)


def can_sym128(shape, tag):
    """... and on the 128 x 128 form it only changes how the diagonal blocks are rounded: every block is computed"""
    return shape == TS_128x128 and tag in (TG_INNER, TG_NEXT)


def can_first_touch(shape, tag):
    return shape == TS_64x64 and tag in (TG_NEXT, TG_BULK, TG_AHEAD)


def modes(c_mode, a_mode=0, b_mode=0, bits=0):
    return c_mode | (a_mode << 2) | (b_mode << 3) | bits


def off(row, col, ld):
    return row * ld + col


def task(c, a, b, klen, m, c_buf=BUF_B, a_buf=BUF_X, b_buf=BUF_KLINV):
    return (c, a, b, klen, c_buf, a_buf, b_buf, m)


def _window(flat, start, nr, nc, pitch):
    """view of nr x nc elements at `start` of a flat buffer, rows `pitch` apart"""
    return np.lib.stride_tricks.as_strided(flat[start:], shape=(nr, nc),
                                           strides=(flat.itemsize * pitch, flat.itemsize), writeable=True)


def operands(bufs, slot, t, ld):
    """A (128 x klen) and B (klen x 128) of task t as the modes address them"""
    c_off, a_off, b_off, klen, c_buf, a_buf, b_buf, m = t
    fa, fb = bufs[slot, a_buf].reshape(-1), bufs[slot, b_buf].reshape(-1)
    A = _window(fa, a_off, klen, TILE, ld).T if (m >> 2) & 1 else _window(fa, a_off, TILE, klen, ld)
    B = _window(fb, b_off, klen, TILE, ld) if (m >> 3) & 1 else _window(fb, b_off, TILE, klen, ld).T
    return A, B


def product(A, B):
    """A.B, exactly: through int64 where the data are integers, else float64 (dyadic data: exact in any order)"""
    if np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B)):
        return (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float64)
    return A @ B


def first_touch_tile(K, s, row0, col0, n):
    """the tile of B = I + D^1/2 K D^1/2 at (row0, col0) as a first touch forms it: delta + (s_m s_n) K_mn inside the
    n x n problem, delta outside (identity padding) -- k_build_B's expression, (s_m * s_n) * K"""
    m = row0 + np.arange(TILE)[:, None]
    c = col0 + np.arange(TILE)[None, :]
    inside = (m < n) & (c < n)
    v = np.where(inside, (s[row0:row0 + TILE, None] * s[None, col0:col0 + TILE]) * K, 0.0)
    return np.where(m == c, v + 1.0, v)


def block_mask(lower):
    """128 x 128 mask of what a task changes: everything, or the 16 x 16 blocks with block column <= block row"""
    if not lower:
        return np.ones((TILE, TILE), dtype=bool)
    b = np.arange(TILE) // 16
    return b[None, :] <= b[:, None]


def written_mask(lower, ft):
    """... and of what it WRITES: under bit 4 the 64 x 64 quarter above the diagonal is not touched at all, and the upper
    blocks of the two diagonal quarters are loaded and stored back -- the same bits, unless the tile is formed on the way
    in (first touch), where they receive the formed tile"""
    if not lower:
        return np.ones((TILE, TILE), dtype=bool)
    w = block_mask(True)
    if ft:
        q = np.arange(TILE) // 64
        w = w | (q[None, :] == q[:, None])
    return w


def apply_launch(bufs, tasks, shape, tag, ldc=0, ft_s=None, ft_n=0):
    """What launch_tiles(tasks, shape, tag) leaves in the buffers.  The entry point's rules hold (C tiles apart from each
    other and from every operand but a task's own), so every task reads the buffers as they came in."""
    nbatch, nbuf, ld, _ = bufs.shape
    out = bufs.copy()
    pitch = ldc if (ldc and tag == TG_COV) else ld
    for slot in range(nbatch):
        for t in tasks:
            c_off, a_off, b_off, klen, c_buf, a_buf, b_buf, m = t
            c_mode = m & 3
            lower = bool(m & LOWER) and can_lower(shape, tag)
            ft = bool(m & FIRST_TOUCH) and ft_s is not None and can_first_touch(shape, tag)
            A, B = operands(bufs, slot, t, ld)
            P = product(A, B)
            C_in = _window(bufs[slot, c_buf].reshape(-1), c_off, TILE, TILE, pitch)
            if ft:
                assert c_mode == CM_SUB
                Kt = _window(bufs[slot, BUF_K].reshape(-1), c_off, TILE, TILE, ld)
                C_in = first_touch_tile(Kt, ft_s[slot], c_off // ld, c_off % ld, ft_n)
            assert not lower or c_mode == CM_SUB              # (a symmetric UPDATE)
            new = {CM_SET: P, CM_SUB: C_in - P, CM_SETNEG: -P}[c_mode]
            res = np.where(block_mask(lower), new, C_in)
            C_out = _window(out[slot, c_buf].reshape(-1), c_off, TILE, TILE, pitch)
            w = written_mask(lower, ft)
            C_out[w] = res[w]
    return out


def apply_panel(bufs, tasks, n_l, acc):
    """k_tile_panel on (nbatch, 2, 256, 256) buffers: every task a product under its modes (the triangular operand carries
    explicit zeros); acc: the first n_l tasks solve x L_kk^T = C in place instead, L_kk the tile at b_off of the task's own
    buffer, the reciprocal pivots the diagonal of the B operand X_kk"""
    nbatch, nbuf, ld, _ = bufs.shape
    out = apply_launch(bufs, tasks[n_l:] if acc else tasks, TS_128x128, TG_MISC)
    if acc:
        for slot in range(nbatch):
            for t in tasks[:n_l]:
                c_off, a_off, b_off, klen, c_buf, a_buf, b_buf, m = t
                L = _window(bufs[slot, a_buf].reshape(-1), b_off, TILE, TILE, ld)
                rinv = np.diag(_window(bufs[slot, b_buf].reshape(-1), b_off, TILE, TILE, ld))
                x = np.array(_window(bufs[slot, c_buf].reshape(-1), c_off, TILE, TILE, ld))
                for c in range(TILE):
                    x[:, c] = (x[:, c] - x[:, :c] @ L[c, :c]) * rinv[c]
                _window(out[slot, c_buf].reshape(-1), c_off, TILE, TILE, ld)[:] = x
    return out


def apply_chain(bufs, which):
    """k_chain_l (which 0): L_10 = B_10 X_00^T in place; k_chain_u (1): the 36 lower 16 x 16 blocks of B_11 -= L_10 L_10^T.
    bufs: (nbatch, 2, 256, 256), B and X."""
    out = bufs.copy()
    for slot in range(bufs.shape[0]):
        Bm, Xm = bufs[slot, 0], bufs[slot, 1]
        if which == 0:
            out[slot, 0, TILE:, :TILE] = product(Bm[TILE:, :TILE], Xm[:TILE, :TILE].T)
        else:
            L = Bm[TILE:, :TILE]
            new = Bm[TILE:, TILE:] - product(L, L.T)
            out[slot, 0, TILE:, TILE:] = np.where(block_mask(True), new, Bm[TILE:, TILE:])
    return out


# ---- data ----------------------------------------------------------------------------------------------------------

def c_rects(tasks, ld, pitch=None):
    pitch = pitch or ld
    return [(t[4], t[0] // pitch, t[0] % pitch) for t in tasks]


def int_bufs(rng, nbatch, ld, tasks=(), ldc=0, nbuf=4):
    """operands in [-4, 4] everywhere, the C tiles of `tasks` in [-9, 9] (unless a task works in place); every slot its own"""
    bufs = rng.randint(-4, 5, size=(nbatch, nbuf, ld, ld)).astype(np.float64)
    for slot in range(nbatch):
        for t in tasks:
            if (t[0], t[4]) in ((t[1], t[5]), (t[2], t[6])):
                continue
            _window(bufs[slot, t[4]].reshape(-1), t[0], TILE, TILE, ldc or ld)[:] = rng.randint(-9, 10, size=(TILE, TILE))
    return bufs


def lower_int(rng, n=TILE, lo=-4, hi=4):
    """lower triangular, explicit (positive) zeros above the diagonal"""
    return np.tril(rng.randint(lo, hi + 1, size=(n, n))).astype(np.float64)


def unit_lower_pair(rng, n=TILE, density=0.25, limit=2.0 ** 53 / (4 * TILE)):
    """L unit lower triangular with entries in {-1, 0, 1} and X = L^-1, an integer matrix.  The entries of L are thinned
    until |X| stays below `limit` (so that X times a 128-term operand in [-4, 4] is exact in float64)."""
    while True:
        L = np.tril(rng.randint(-1, 2, size=(n, n)) * (rng.rand(n, n) < density), -1) + np.eye(n, dtype=np.int64)
        X = np.zeros((n, n), dtype=object)
        for i in range(n):                                   # row i of L^-1 by forward substitution, Python integers
            row = -sum((int(L[i, j]) * X[j] for j in np.nonzero(L[i, :i])[0]), np.zeros(n, dtype=object))
            row[i] += 1
            X[i] = row
        if max(abs(v) for v in X.reshape(-1)) < limit:
            return L.astype(np.float64), X.astype(np.float64)
        density *= 0.7


def seeds(rng, shape):
    """values for memory a launch must not change: magnitudes from subnormal to huge, both signs, full mantissas (no
    -0.0: a sign round trip of +0.0 would show, one of -0.0 would not)"""
    v = rng.uniform(1.0, 2.0, size=shape) * 2.0 ** rng.randint(-1070, 1020, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    v[rng.rand(*shape) < 0.05] = 0.0
    return v


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---- the accumulate-from-zero form, to the bit ----------------------------------------------------------------------
# Operands i 2^-28 with |i| <= 256, C uniform in [1, 2) with full mantissas: S = A.B is a multiple of 2^-56 below 2^-30,
# exact in any order, and C - S a multiple of 2^-56 below 2: everything fits int64 in units of 2^-56.

SYM_UNIT = 2.0 ** -56


def sym_operand(rng, shape):
    return rng.randint(-256, 257, size=shape) * 2.0 ** -28


def sym_c(rng, shape):
    return 1.0 + rng.randint(0, 2 ** 52, size=shape, dtype=np.int64) * 2.0 ** -52


def to_units(x):
    """a float64 array of multiples of 2^-56 (below 2^6) as int64 counts, exactly"""
    u = x * 2.0 ** 56
    assert np.array_equal(u, np.rint(u)) and np.abs(u).max() < 2.0 ** 62
    return u.astype(np.int64)


def exact_c_minus_ab(C, A, B):
    """C - A.B in units of 2^-56, exact (int64)"""
    ia, ib = A * 2.0 ** 28, B * 2.0 ** 28                          # the integers i
    assert np.array_equal(ia, np.rint(ia)) and np.array_equal(ib, np.rint(ib))
    return to_units(C) - ia.astype(np.int64) @ ib.astype(np.int64)


def rounded(units):
    """fl(units 2^-56): int64 -> float64 rounds to nearest even, the scaling is exact"""
    return units.astype(np.float64) * SYM_UNIT


def in_accumulator_form(C, A, B):
    """what the tile kernel's other blocks do: acc = -C, acc += four products at a time, C = -acc -- one rounding at C's
    magnitude per MFMA step (a sum of four products of this data is exact)"""
    acc = -C
    for k in range(0, A.shape[1], 4):
        acc = acc + A[:, k:k + 4] @ B[k:k + 4, :]
    return -acc


# ---- task geometry shared by the tests ------------------------------------------------------------------------------

def may_change(shape_of_bufs, tasks, shape, tag, ldc=0, ft=False):
    """boolean array over the buffers: the elements a launch may write other bits to"""
    nbatch, nbuf, ld, _ = shape_of_bufs
    pitch = ldc if (ldc and tag == TG_COV) else ld
    m = np.zeros(shape_of_bufs, dtype=bool)
    for t in tasks:
        lower = bool(t[7] & LOWER) and can_lower(shape, tag)
        w = written_mask(lower, ft and bool(t[7] & FIRST_TOUCH)) if ft else block_mask(lower)
        for slot in range(nbatch):
            _window(m[slot, t[4]].reshape(-1), t[0], TILE, TILE, pitch)[w] = True
    return m


def operand_off(ld, klen, mode, i):
    """where task i's operand lies: 128 rows x klen columns inside tile row 0 (mode 0), or klen rows x 128 columns inside
    tile column 0 (mode 1) -- never inside a tile (r, c) with r, c >= 1, where the C tiles are"""
    if mode == 0:
        c0 = (0, ld - klen, min(2, ld - klen))[i % 3]
        return off(0, c0, ld)
    return off(0, 0, ld)


def c_tile_off(ld, i):
    """the i-th C tile: tiles (r, c) with r, c >= 1, last one first"""
    T = ld // TILE
    r, c = divmod(i, T - 1)
    return off((T - 1 - r) * TILE, (T - 1 - c) * TILE, ld)


def lower_tasks(ld, klen, own_pitch):
    """two diagonal tasks (bit 4: C -= A A^T, the same operand twice) and an off-diagonal one between them, one launch"""
    ldc, c_buf = (ld + 128, BUF_K) if own_pitch else (ld, BUF_B)
    a0, a1 = off(0, 0, ld), off(0, ld - klen, ld)
    # (own pitch: side by side in rows of ldc, the third one a hundred rows further down)
    cs = [off(128, 128, ldc), off(128, 0, ldc), off(256, 256, ldc)] if not own_pitch else \
        [off(0, 0, ldc), off(0, 128, ldc), off(100, 256, ldc)]
    return [task(cs[0], a0, a0, klen, modes(CM_SUB, 0, 0, LOWER), c_buf, BUF_X, BUF_X),
            task(cs[1], a0, a1, klen, modes(CM_SUB, 0, 0), c_buf, BUF_X, BUF_KLINV),
            task(cs[2], a1, a1, klen, modes(CM_SUB, 0, 0, LOWER), c_buf, BUF_KLINV, BUF_KLINV)]


SYM_FORMS = [(TS_64x64, t) for t in (TG_INNER, TG_NEXT, TG_BULK, TG_AHEAD, TG_COV)] + [(TS_128x128, TG_INNER), (TS_128x128, TG_NEXT)]
SYM_KLENS = [128, 512]


def sym_case(shape, tag, klen, ld=512, nbatch=2):
    """the launch of test_sym_accumulates_from_zero: (bufs, tasks, ldc)"""
    own = tag == TG_COV
    rng = np.random.RandomState(6000 + 64 * shape + 8 * tag + klen)
    tasks = lower_tasks(ld, klen, own)
    bufs = sym_operand(rng, (nbatch, 4, ld, ld))
    bufs[:, tasks[0][4]] = sym_c(rng, (nbatch, ld, ld))
    return bufs, tasks, (ld + 128 if own else 0)


def sym_chain_case(table, nbatch=3):
    """... and of test_chain_u_accumulates_from_zero: B_11 in [1, 2), everything else dyadic operands"""
    rng = np.random.RandomState(8200 + table)
    bufs = sym_operand(rng, (nbatch, 2, 2 * TILE, 2 * TILE))
    bufs[:, BUF_B, TILE:, TILE:] = sym_c(rng, (nbatch, TILE, TILE))
    return bufs
