"""Every instantiation of the tile kernels, ONE launch at a time, against the NumPy model of a launch (tests/_tile_ref.py).

gprn_test_tile_launch / gprn_test_tile_step run one launch on the test's own buffers and task list and return every
buffer of every slot in full.  The data are small integers (every product and partial sum representable: the result has
the same bits in any summation order) or dyadic fractions (the accumulate-from-zero form, to the bit), so every assertion
is an equality over the WHOLE buffers: a wrong element, a skipped chunk, a stray write anywhere fails the launch that did
it, by name.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

from gpyrn_amd import _hip
from tests import _tile_ref as R

pytestmark = pytest.mark.gpu

MODE_PAIRS = [(0, 0), (0, 1), (1, 1), (1, 0)]
KLENS = [16, 32, 48, 64, 80, 128, 512]


@pytest.fixture(scope='module')
def ctx():
    c = _hip.Context(0)
    yield c
    c.close()


def where(got, want):
    bad = np.argwhere(got != want)
    return '%d elements differ, the first at (slot, buffer, row, column) = %s: got %r, want %r' % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else 'bits differ'


def check_launch(ctx, bufs, tasks, shape, tag, untouched_bits=False, **kw):
    """one launch against the model: equal over the whole buffers; untouched_bits: and not a bit changed outside what the
    tasks may write"""
    got = ctx.test_tile_launch(bufs, tasks, shape, tag, **kw)
    want = R.apply_launch(bufs, tasks, shape, tag, ldc=kw.get('ldc', 0), ft_s=kw.get('ft_s'), ft_n=kw.get('ft_n', 0))
    assert np.array_equal(got, want), where(got, want)
    if untouched_bits:
        keep = ~R.may_change(bufs.shape, tasks, shape, tag, kw.get('ldc', 0), ft=kw.get('ft_s') is not None)
        assert R.same_bits(got[keep], bufs[keep]), 'memory outside the written blocks changed its bits'
    return got


def triangular(bufs, buf, at, ld, upper):
    """the 128 x 128 stored at `at` of every slot's buffer `buf` becomes triangular, explicit zeros in the other half"""
    for slot in range(bufs.shape[0]):
        w = R._window(bufs[slot, buf].reshape(-1), at, R.TILE, R.TILE, ld)
        w[:] = np.triu(w) if upper else np.tril(w)


# ---- every instantiation of launch_tiles' switch -------------------------------------------------------------------

@pytest.mark.parametrize('pair', R.PAIRS, ids=R.pair_id)
def test_every_instantiation(ctx, pair):
    """three tasks, three slots, every a_mode / b_mode pair and c_mode: C tiles in three different buffers, operands at
    different offsets, klen 32 / 80 / 128 in ONE launch (the triangular forms: 128, X_kk with explicit zeros)"""
    shape, tag = pair
    ld, nbatch = 256, 3
    tri = {R.TS_64x128_BTRI: 'b', R.TS_128x64_ATRI: 'a'}.get(shape)
    rng = np.random.RandomState(1000 + 8 * shape + tag)
    for ldc in ([0, 384] if tag == R.TG_COV else [0]):
        for a_mode, b_mode in MODE_PAIRS:
            for c_mode in (R.CM_SET, R.CM_SUB, R.CM_SETNEG):
                tasks = []
                for i, klen in enumerate([128] * 3 if tri else [32, 80, 128]):
                    a = R.off(0, 128 * (i % 2), ld) if (tri == 'a' and a_mode == 0) else R.operand_off(ld, klen, a_mode, i)
                    b = R.off(0, 128 * (i % 2), ld) if (tri == 'b' and b_mode == 0) else R.operand_off(ld, klen, b_mode, i + 1)
                    if ldc:
                        c, c_buf = 128 * i, R.BUF_K                 # side by side in rows of 384, a buffer of their own
                    else:
                        c, c_buf = R.c_tile_off(ld, 0), (R.BUF_B, R.BUF_K, R.BUF_X)[i]
                    tasks.append(R.task(c, a, b, klen, R.modes(c_mode, a_mode, b_mode), c_buf=c_buf))
                bufs = R.int_bufs(rng, nbatch, ld, tasks, ldc)
                for t in tasks:
                    if tri == 'a':
                        triangular(bufs, t[5], t[1], ld, upper=a_mode == 1)    # A(m, k) = 0 for k > m
                    if tri == 'b':
                        triangular(bufs, t[6], t[2], ld, upper=b_mode == 1)    # B(k, n) = 0 for k > n
                check_launch(ctx, bufs, tasks, shape, tag, ldc=ldc)


# ---- the K pipeline's edges ---------------------------------------------------------------------------------------

PIPE_FORMS = [(R.TS_64x64, R.TG_BULK), (R.TS_64x64, R.TG_MISC), (R.TS_64x128, R.TG_MISC), (R.TS_128x64, R.TG_MISC),
              (R.TS_128x128, R.TG_MISC), (R.TS_128x128, R.TG_BULK)]


@pytest.mark.parametrize('klen', KLENS + ['mixed'])
@pytest.mark.parametrize('pair', PIPE_FORMS, ids=R.pair_id)
def test_pipeline_edges(ctx, pair, klen):
    """one chunk, two chunks (the reloads of the last chunk), odd and even counts (the two tails of the two-register-set
    form), the factorisation's own 128 and 512 -- one launch per klen, and one launch that carries them all"""
    shape, tag = pair
    ld, nbatch = 512, 2
    rng = np.random.RandomState(2000 + 8 * shape + tag + (999 if klen == 'mixed' else klen))
    klens = KLENS if klen == 'mixed' else [klen, klen]
    tasks = []
    for i, k in enumerate(klens):
        a_mode, b_mode = MODE_PAIRS[(i + (0 if klen == 'mixed' else 2 * (k // 16))) % 4]
        tasks.append(R.task(R.c_tile_off(ld, i), R.operand_off(ld, k, a_mode, i), R.operand_off(ld, k, b_mode, i + 1), k,
                            R.modes(R.CM_SUB, a_mode, b_mode)))
    bufs = R.int_bufs(rng, nbatch, ld, tasks)
    check_launch(ctx, bufs, tasks, shape, tag)


# ---- TRI: the skipped K-chunks, the in-place panel tasks ------------------------------------------------------------

@pytest.mark.parametrize('c_mode', [R.CM_SET, R.CM_SETNEG])
@pytest.mark.parametrize('shape', [R.TS_64x128_BTRI, R.TS_128x64_ATRI], ids=['64x128_BTRI', '128x64_ATRI'])
def test_tri_in_place(ctx, shape, c_mode):
    """L_ik = B_ik X_kk^T over B_ik (C tile == A operand, 64 x 128) and X_kc = X_kk R_kc over R_kc (C tile == B operand,
    128 x 64): the result is the dense product, and nothing else in the four buffers moves"""
    ld, nbatch = 256, 3
    rng = np.random.RandomState(3000 + 4 * shape + c_mode)
    xkk = R.off(0, 0, ld)
    if shape == R.TS_64x128_BTRI:
        tasks = [R.task(R.off(128, 0, ld), R.off(128, 0, ld), xkk, 128, R.modes(c_mode, 0, 0), R.BUF_B, R.BUF_B, R.BUF_X),
                 R.task(R.off(128, 128, ld), R.off(128, 128, ld), xkk, 128, R.modes(c_mode, 0, 0), R.BUF_B, R.BUF_B, R.BUF_X),
                 R.task(R.off(0, 128, ld), R.off(0, 0, ld), xkk, 128, R.modes(c_mode, 0, 0), R.BUF_K, R.BUF_B, R.BUF_X)]
    else:
        tasks = [R.task(R.off(128, 0, ld), xkk, R.off(128, 0, ld), 128, R.modes(c_mode, 0, 1), R.BUF_X, R.BUF_X, R.BUF_X),
                 R.task(R.off(128, 128, ld), xkk, R.off(128, 128, ld), 128, R.modes(c_mode, 0, 1), R.BUF_X, R.BUF_X, R.BUF_X),
                 R.task(R.off(0, 128, ld), xkk, R.off(0, 0, ld), 128, R.modes(c_mode, 0, 1), R.BUF_K, R.BUF_X, R.BUF_B)]
    bufs = R.int_bufs(rng, nbatch, ld, tasks)
    triangular(bufs, R.BUF_X, xkk, ld, upper=False)
    check_launch(ctx, bufs, tasks, shape, R.TG_PANEL)


def panel_tasks(n_l, n_x, ld=256):
    """a tile step's panel at 256: L tasks over tiles (1, 0), (1, 1) of B in place, X tasks over tiles (1, 0), (1, 1) of X
    in place, all against X_00"""
    xkk = R.off(0, 0, ld)
    lt = [R.task(R.off(128, 128 * j, ld), R.off(128, 128 * j, ld), xkk, 128, R.modes(R.CM_SET, 0, 0), R.BUF_B, R.BUF_B, R.BUF_X)
          for j in range(n_l)]
    xt = [R.task(R.off(128, 128 * j, ld), xkk, R.off(128, 128 * j, ld), 128, R.modes((R.CM_SET, R.CM_SETNEG)[j], 0, 1),
                 R.BUF_X, R.BUF_X, R.BUF_X) for j in range(n_x)]
    return lt + xt


@pytest.mark.parametrize('n_l,n_x', [(2, 2), (1, 1), (2, 0), (0, 2)])
def test_panel_products(ctx, n_l, n_x):
    """k_tile_panel<false>: both halves of a panel in one launch, either half empty"""
    rng = np.random.RandomState(3100 + 4 * n_l + n_x)
    tasks = panel_tasks(n_l, n_x)
    bufs = R.int_bufs(rng, 3, 256, nbuf=2)
    triangular(bufs, R.BUF_X, 0, 256, upper=False)
    got = ctx.test_tile_step(bufs, 2, tasks=tasks, n_l=n_l)
    want = R.apply_panel(bufs, tasks, n_l, acc=False)
    assert np.array_equal(got, want), where(got, want)


@pytest.fixture(scope='module')
def unit_pair():
    return R.unit_lower_pair(np.random.RandomState(3200))


def subst_bufs(rng, unit_pair, nbatch, nbuf):
    """L_00 unit lower with entries in {-1, 0, 1} (above its diagonal: values a solve must not read), X_00 its integer
    inverse, tiles (1, 0) and (1, 1) of B the right-hand sides Y L_00^T of small-integer Y"""
    L, X = unit_pair
    bufs = R.int_bufs(rng, nbatch, 256, nbuf=nbuf)
    Y = rng.randint(-4, 5, size=(nbatch, 2, 128, 128)).astype(np.float64)
    for slot in range(nbatch):
        bufs[slot, R.BUF_B, :128, :128] = L + np.triu(R.seeds(rng, (128, 128)), 1)
        bufs[slot, R.BUF_X, :128, :128] = X
        for j in range(2):
            rhs = Y[slot, j] @ L.T
            assert np.abs(rhs).max() < 2.0 ** 53
            bufs[slot, R.BUF_B, 128:, 128 * j:128 * (j + 1)] = rhs
    return bufs, Y


@pytest.mark.parametrize('n_l,n_x', [(2, 2), (1, 1), (1, 0), (2, 0), (0, 2)])
def test_panel_substitution(ctx, unit_pair, n_l, n_x):
    """k_tile_panel<true>: the L part solves x L_00^T = b by substitution.  Every intermediate of any substitution order is
    a small integer and the reciprocal pivots are exactly 1: Y comes back exactly."""
    rng = np.random.RandomState(3300 + 4 * n_l + n_x)
    bufs, Y = subst_bufs(rng, unit_pair, 3, 2)
    tasks = panel_tasks(n_l, n_x)
    got = ctx.test_tile_step(bufs, 3, tasks=tasks, n_l=n_l)
    for j in range(n_l):
        assert np.array_equal(got[:, R.BUF_B, 128:, 128 * j:128 * (j + 1)], Y[:, j])
    want = R.apply_panel(bufs, tasks, n_l, acc=True)
    assert np.array_equal(got, want), where(got, want)


def test_panel_substitution_through_launch_tiles(ctx, unit_pair):
    """... and as launch_tiles reaches it: TS_64x128_BTRI / TG_PANEL with the substitution flag"""
    rng = np.random.RandomState(3400)
    bufs, Y = subst_bufs(rng, unit_pair, 3, 4)
    tasks = panel_tasks(2, 0)
    got = ctx.test_tile_launch(bufs, tasks, R.TS_64x128_BTRI, R.TG_PANEL, acc=True)
    want = bufs.copy()
    want[:, R.BUF_B, 128:, :128], want[:, R.BUF_B, 128:, 128:] = Y[:, 0], Y[:, 1]
    assert np.array_equal(got, want), where(got, want)


# ---- LOWER: the symmetric update of a diagonal tile ----------------------------------------------------------------

LOWER_TAGS = [R.TG_INNER, R.TG_NEXT, R.TG_BULK, R.TG_AHEAD, R.TG_COV]


@pytest.mark.parametrize('tag', LOWER_TAGS, ids=[R.TAG_NAMES[t] for t in LOWER_TAGS])
def test_lower_blocks_only(ctx, tag):
    """bit 4 on the 64 x 64 form: the 36 lower 16 x 16 blocks are updated, the 28 others keep their bits -- values from
    subnormal to huge that a sign round trip or a rewrite would show -- in a launch that mixes diagonal and off-diagonal
    tasks"""
    ld, nbatch = 384, 3
    own = tag == R.TG_COV
    rng = np.random.RandomState(4000 + tag)
    for klen in (128, 384) if tag != R.TG_INNER else (128,):
        tasks = R.lower_tasks(ld, klen, own)
        ldc = ld + 128 if own else 0
        bufs = R.int_bufs(rng, nbatch, ld, tasks, ldc)
        upper = ~R.block_mask(True)
        for slot in range(nbatch):
            for t in tasks:
                if t[7] & R.LOWER:
                    R._window(bufs[slot, t[4]].reshape(-1), t[0], 128, 128, ldc or ld)[upper] = R.seeds(rng, (128, 128))[upper]
        check_launch(ctx, bufs, tasks, R.TS_64x64, tag, untouched_bits=True, ldc=ldc)


# ---- first touch: the tile of B = I + D^1/2 K D^1/2 formed on the way in ---------------------------------------------

FT_TAGS = [R.TG_NEXT, R.TG_BULK, R.TG_AHEAD]
FT_N = [256, 232, 129, 128, 1]                # tiles wholly inside, straddling, wholly outside the problem (ld = 256)


def ft_tasks(ld, klen, lower_at, plain_at=None, zero_a=()):
    """the four tiles of B: both diagonal ones (bit 4 on `lower_at`, same operand twice), both off-diagonal ones; all
    first touches but `plain_at`.  A from BUF_X, B from BUF_KLINV; zero_a: tasks whose A lies at the far right of BUF_X"""
    tasks = []
    for i, (r, c) in enumerate([(0, 0), (1, 1), (1, 0), (0, 1)]):
        bits = (R.LOWER if (r, c) == lower_at else 0) | (0 if (r, c) == plain_at else R.FIRST_TOUCH)
        a = R.off(0, ld - klen if i in zero_a else 2 * i, ld)
        b = R.off(0, 2 * i + 32, ld)
        if (r, c) == lower_at:
            tasks.append(R.task(R.off(128 * r, 128 * c, ld), b, b, klen, R.modes(R.CM_SUB, 0, 0, bits), R.BUF_B, R.BUF_KLINV, R.BUF_KLINV))
        else:
            tasks.append(R.task(R.off(128 * r, 128 * c, ld), a, b, klen, R.modes(R.CM_SUB, 0, 0, bits)))
    return tasks


@pytest.mark.parametrize('ft_n', FT_N)
@pytest.mark.parametrize('tag', FT_TAGS, ids=[R.TAG_NAMES[t] for t in FT_TAGS])
def test_first_touch_exact(ctx, tag, ft_n):
    """integer K, power-of-two s (every slot its own): delta + (s_m s_n) K inside the ft_n x ft_n problem, delta outside,
    whatever B held before (values that would show if it were read); with bit 4 and without, beside a task that is no
    first touch"""
    ld, nbatch = 256, 3
    rng = np.random.RandomState(5000 + 16 * tag + ft_n)
    for lower_at, plain_at in (((0, 0), (0, 1)), ((1, 1), None)):
        tasks = ft_tasks(ld, 48, lower_at, plain_at)
        bufs = R.int_bufs(rng, nbatch, ld, tasks)
        for slot in range(nbatch):
            for t in tasks:
                if t[7] & R.FIRST_TOUCH:
                    R._window(bufs[slot, R.BUF_B].reshape(-1), t[0], 128, 128, ld)[:] = R.seeds(rng, (128, 128))
        s = 2.0 ** rng.randint(-3, 4, size=(nbatch, ld))
        check_launch(ctx, bufs, tasks, R.TS_64x64, tag, untouched_bits=True, ft_s=s, ft_n=ft_n)


@pytest.mark.parametrize('ft_n', FT_N)
@pytest.mark.parametrize('tag', FT_TAGS, ids=[R.TAG_NAMES[t] for t in FT_TAGS])
def test_first_touch_rounds_as_build_B(ctx, tag, ft_n):
    """random float64 K and s: the launch with bit 5 against the SAME launch without it on a B that NumPy filled with
    delta + (s_m * s_n) * K_mn -- the order k_build_B uses -- bit for bit.  klen = 16; the tasks without bit 4 have A = 0
    (their result IS the incoming tile), the one with bit 4 a random operand (its diagonal blocks take the tile in at the
    end).  A difference on diagonal entries only would mean that the + 1.0 is contracted into an FMA on one side."""
    ld, nbatch, klen = 256, 3, 16
    rng = np.random.RandomState(5500 + 16 * tag + ft_n)
    tasks = ft_tasks(ld, klen, (1, 1), zero_a=(0, 2, 3))
    bufs = rng.standard_normal((nbatch, 4, ld, ld))
    bufs[:, R.BUF_X, :128, ld - klen:] = 0.0
    bufs[:, R.BUF_B] = R.seeds(rng, (nbatch, ld, ld))
    s = rng.uniform(0.5, 2.0, size=(nbatch, ld))
    got = ctx.test_tile_launch(bufs, tasks, R.TS_64x64, tag, ft_s=s, ft_n=ft_n)
    filled = bufs.copy()
    for slot in range(nbatch):
        for t in tasks:
            r0, c0 = divmod(t[0], ld)
            filled[slot, R.BUF_B, r0:r0 + 128, c0:c0 + 128] = R.first_touch_tile(
                bufs[slot, R.BUF_K, r0:r0 + 128, c0:c0 + 128], s[slot], r0, c0, ft_n)
    plain = [t[:7] + (t[7] & ~R.FIRST_TOUCH,) for t in tasks]
    ref = ctx.test_tile_launch(filled, plain, R.TS_64x64, tag)
    written = R.may_change(bufs.shape, tasks, R.TS_64x64, tag, ft=True)
    for slot in range(nbatch):
        for t in tasks:
            r0, c0 = divmod(t[0], ld)
            g, w = got[slot, R.BUF_B, r0:r0 + 128, c0:c0 + 128], ref[slot, R.BUF_B, r0:r0 + 128, c0:c0 + 128]
            m = written[slot, R.BUF_B, r0:r0 + 128, c0:c0 + 128]
            differ = m & (g.view(np.int64) != w.view(np.int64))
            assert not differ.any(), 'tile (%d, %d), slot %d: %d entries differ, %d of them on the diagonal' % (
                r0 // 128, c0 // 128, slot, differ.sum(), np.diag(differ).sum() if r0 == c0 else 0)
    assert R.same_bits(got[~written], bufs[~written])


# ---- SYM: the diagonal blocks accumulate from zero, to the bit -----------------------------------------------------

SYM_FORMS = [(R.TS_64x64, t) for t in LOWER_TAGS] + [(R.TS_128x128, R.TG_INNER), (R.TS_128x128, R.TG_NEXT)]
DIAG_BLOCKS = (np.arange(128)[:, None] // 16) == (np.arange(128)[None, :] // 16)


@pytest.mark.parametrize('klen', [128, 512])
@pytest.mark.parametrize('pair', SYM_FORMS, ids=R.pair_id)
def test_sym_accumulates_from_zero(ctx, pair, klen):
    """operands i 2^-28, C in [1, 2) with full mantissas: A.B is exact in any order, so the diagonal 16 x 16 blocks of a
    bit-4 task must hold fl(C - A.B) exactly -- one rounding.  With the tile in the accumulator from the start they would
    not (tests/test_tile_ref.py shows that this data tells the two apart).  Every other computed block rounds once per MFMA
    step at most: |err| <= (klen / 4 + 1) 2^-52."""
    shape, tag = pair
    ld, nbatch = 512, 2
    bufs, tasks, ldc = R.sym_case(shape, tag, klen)
    c_buf = tasks[0][4]
    got = ctx.test_tile_launch(bufs, tasks, shape, tag, ldc=ldc)
    keep = np.ones(bufs.shape, dtype=bool)
    bound = (klen // 4 + 1) * 16                              # in units of 2^-56
    for slot in range(nbatch):
        for t in tasks:
            A, B = R.operands(bufs, slot, t, ld)
            C = R._window(bufs[slot, c_buf].reshape(-1), t[0], 128, 128, ldc or ld)
            G = R._window(got[slot, c_buf].reshape(-1), t[0], 128, 128, ldc or ld)
            exact = R.exact_c_minus_ab(C, A, B)
            sym = bool(t[7] & R.LOWER)
            computed = R.block_mask(sym and R.can_lower(shape, tag))
            R._window(keep[slot, c_buf].reshape(-1), t[0], 128, 128, ldc or ld)[computed] = False
            if sym:
                assert R.same_bits(G[DIAG_BLOCKS], R.rounded(exact)[DIAG_BLOCKS]), \
                    'task at %d, slot %d: a diagonal block is not fl(C - A.B)' % (t[0], slot)
            err = np.abs(R.to_units(np.where(computed, G, 0.0)) - np.where(computed, exact, 0))
            assert err.max() <= bound, (int(err.max()), bound)
    assert R.same_bits(got[keep], bufs[keep]), 'memory outside the computed blocks changed its bits'


# ---- the XCD re-map: a bijection of the workgroups --------------------------------------------------------------------

@pytest.mark.parametrize('ntasks,nbatch', [(33, 1), (33, 2), (31, 1)], ids=['132wg', '264wg-two-slots', '124wg-unmapped'])
def test_xcd_remap_is_a_bijection(ctx, ntasks, nbatch):
    """64 x 64 workgroups, four per task: 132 (128 re-mapped, 4 not), 264 over two slots (256 re-mapped, positions that
    cross the slot boundary), 124 (none).  Every tile of every slot is updated exactly once, each from its own data."""
    ld = 768
    rng = np.random.RandomState(7000 + ntasks + nbatch)
    tasks = []
    for i in range(ntasks):
        r, c = divmod(i, 6)
        tasks.append(R.task(R.off(128 * r, 128 * c, ld), R.off(128 * (i % 6), 16 * (i % 7), ld),
                            R.off(128 * (i % 5), 16 * (i % 11), ld), 32, R.modes(R.CM_SUB, 0, 0)))
    bufs = R.int_bufs(rng, nbatch, ld, tasks)
    for tag in (R.TG_BULK, R.TG_MISC):
        check_launch(ctx, bufs, tasks, R.TS_64x64, tag)


# ---- the latency chain's two products ---------------------------------------------------------------------------------

CHAIN_CASES = [(1, 1), (1, 0), (3, 1), (3, 0), (16, 1), (16, 0), (18, 1)]


def chain_ids(v):
    return '%d-%s' % (v[0], 'args' if v[1] and v[0] <= 16 else 'table')


@pytest.mark.parametrize('case', CHAIN_CASES, ids=chain_ids)
def test_chain_l(ctx, case):
    """k_chain_l: L_10 = B_10 X_00^T in place over B_10, pointers as kernel arguments and from the table"""
    nbatch, table = case
    rng = np.random.RandomState(8000 + 2 * nbatch + table)
    bufs = R.int_bufs(rng, nbatch, 256, nbuf=2)
    triangular(bufs, R.BUF_X, 0, 256, upper=False)
    got = ctx.test_tile_step(bufs, 0, table=table)
    want = R.apply_chain(bufs, 0)
    assert np.array_equal(got, want), where(got, want)


@pytest.mark.parametrize('case', CHAIN_CASES, ids=chain_ids)
def test_chain_u(ctx, case):
    """k_chain_u: the 36 lower blocks of B_11 -= L_10 L_10^T; the 28 upper ones keep their bits"""
    nbatch, table = case
    rng = np.random.RandomState(8100 + 2 * nbatch + table)
    bufs = R.int_bufs(rng, nbatch, 256, nbuf=2)
    bufs[:, R.BUF_B, 128:, 128:] = rng.randint(-9, 10, size=(nbatch, 128, 128))
    upper = ~R.block_mask(True)
    bufs[:, R.BUF_B, 128:, 128:][:, upper] = R.seeds(rng, (nbatch, 128, 128))[:, upper]
    got = ctx.test_tile_step(bufs, 1, table=table)
    want = R.apply_chain(bufs, 1)
    assert np.array_equal(got, want), where(got, want)
    assert R.same_bits(got[:, R.BUF_B, 128:, 128:][:, upper], bufs[:, R.BUF_B, 128:, 128:][:, upper])


@pytest.mark.parametrize('table', [1, 0], ids=['args', 'table'])
def test_chain_u_accumulates_from_zero(ctx, table):
    """... and all 36 hold fl(C - L L^T) exactly on the dyadic data (k_chain_u subtracts once, at the end)"""
    nbatch = 3
    bufs = R.sym_chain_case(table)
    got = ctx.test_tile_step(bufs, 1, table=table)
    want = bufs.copy()
    lower = R.block_mask(True)
    for slot in range(nbatch):
        L = bufs[slot, R.BUF_B, 128:, :128]
        new = R.rounded(R.exact_c_minus_ab(bufs[slot, R.BUF_B, 128:, 128:], L, L.T))
        want[slot, R.BUF_B, 128:, 128:] = np.where(lower, new, bufs[slot, R.BUF_B, 128:, 128:])
    assert R.same_bits(got, want), where(got, want)


# ---- refusals: every rule stops on the host ------------------------------------------------------------------------

def good_launch(ld=256):
    return dict(tasks=[R.task(R.off(128, 128, ld), R.off(0, 0, ld), R.off(0, 64, ld), 64, R.modes(R.CM_SUB, 0, 0))],
                shape=R.TS_64x64, tag=R.TG_BULK)


def with_task(**changes):
    names = ['c_off', 'a_off', 'b_off', 'klen', 'c_buf', 'a_buf', 'b_buf', 'modes']
    g = good_launch()
    t = list(g['tasks'][0])
    extra = {}
    for k, v in changes.items():
        if k in names:
            t[names.index(k)] = v
        else:
            extra[k] = v
    g['tasks'] = [tuple(t)]
    g.update(extra)
    return g


REFUSALS = {
    'klen-not-a-multiple-of-16': (with_task(klen=24), 'klen'),
    'klen-zero': (with_task(klen=0), 'klen'),
    'buffer-index': (with_task(b_buf=4), 'buffer index'),
    'a-leaves-its-buffer': (with_task(a_off=R.off(0, 224, 256)), 'A operand leaves'),
    'b-leaves-its-buffer': (with_task(b_off=R.off(192, 0, 256)), 'B operand leaves'),
    'b-mode-1-leaves-its-buffer': (with_task(b_off=R.off(224, 0, 256), modes=R.modes(R.CM_SUB, 0, 1)), 'B operand leaves'),
    'c-leaves-its-buffer': (with_task(c_off=R.off(192, 0, 256)), 'C tile leaves'),
    'c-leaves-its-row': (with_task(c_off=R.off(0, 192, 256)), 'C tile leaves'),
    'c-own-pitch-leaves-its-buffer': (with_task(c_off=R.off(64, 0, 384), c_buf=R.BUF_K, tag=R.TG_COV, ldc=384), 'C tile leaves'),
    'ldc-without-cov': (with_task(ldc=384), 'ldc'),
    'unknown-shape-tag': (with_task(shape=R.TS_64x128, tag=R.TG_BULK), 'shape/tag'),
    'bit-5-without-ft_s': (with_task(modes=R.modes(R.CM_SUB, 0, 0, R.FIRST_TOUCH)), 'bit 5'),
    'bit-5-with-cm-set': (with_task(modes=R.modes(R.CM_SET, 0, 0, R.FIRST_TOUCH), ft_s=np.ones((1, 256)), ft_n=256), 'bit 5'),
    'c-is-an-operand': (with_task(c_off=R.off(0, 0, 256), c_buf=R.BUF_X), 'overlaps an operand'),
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals(ctx, name):
    """one broken rule per case: GPRN_E_ARG with a text and nothing launched; the next good call is right, and no call
    fell back to the event schedule"""
    kw, text = REFUSALS[name]
    rng = np.random.RandomState(9000)
    before = ctx.option('fallbacks')
    bufs = R.int_bufs(rng, 1, 256)
    with pytest.raises(_hip.BackendError, match=text + r'.*\(code -1\)'):
        ctx.test_tile_launch(bufs, **kw)
    g = good_launch()
    check_launch(ctx, R.int_bufs(rng, 1, 256, g['tasks']), **g)
    assert ctx.option('fallbacks') == before


def test_refusals_of_whole_launches(ctx):
    rng = np.random.RandomState(9001)
    before = ctx.option('fallbacks')
    g = good_launch()
    with pytest.raises(_hip.BackendError, match=r'multiple of 128.*\(code -1\)'):
        ctx.test_tile_launch(R.int_bufs(rng, 1, 192), **g)
    two = [g['tasks'][0], g['tasks'][0][:1] + (R.off(0, 16, 256),) + g['tasks'][0][2:]]
    with pytest.raises(_hip.BackendError, match=r'C tile overlaps another.*\(code -1\)'):
        ctx.test_tile_launch(R.int_bufs(rng, 1, 256), two, g['shape'], g['tag'])
    half = [g['tasks'][0], (R.off(64, 128, 256),) + g['tasks'][0][1:]]
    with pytest.raises(_hip.BackendError, match=r'C tile overlaps another.*\(code -1\)'):
        ctx.test_tile_launch(R.int_bufs(rng, 1, 256), half, g['shape'], g['tag'])
    step = R.int_bufs(rng, 2, 256, nbuf=2)
    with pytest.raises(_hip.BackendError, match=r'which.*\(code -1\)'):
        ctx.test_tile_step(step, 4)
    with pytest.raises(_hip.BackendError, match=r'buffer index.*\(code -1\)'):
        ctx.test_tile_step(step, 2, tasks=[t[:6] + (R.BUF_K,) + t[7:] for t in panel_tasks(1, 0)], n_l=1)
    with pytest.raises(_hip.BackendError, match=r'klen = 128.*\(code -1\)'):
        ctx.test_tile_step(step, 2, tasks=[t[:3] + (64,) + t[4:] for t in panel_tasks(1, 0)], n_l=1)
    with pytest.raises(_hip.BackendError, match=r'works in place.*\(code -1\)'):
        ctx.test_tile_step(step, 3, tasks=[(R.off(128, 128, 256),) + t[1:] for t in panel_tasks(1, 0)], n_l=1)
    check_launch(ctx, R.int_bufs(rng, 1, 256, g['tasks']), **g)
    assert ctx.option('fallbacks') == before
