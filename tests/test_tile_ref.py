"""The NumPy model of a tile launch (tests/_tile_ref.py) against plain NumPy, and the conditions on the data of
tests/test_tiles_gpu.py that make its equalities mean something.  No GPU."""
import numpy as np
import pytest

from tests import _tile_ref as R


def _plain_operand(buf, at, klen, mode, ld):
    """operand of a task by slicing: 128 x klen stored as is (mode 0) or klen x 128 (mode 1)"""
    r, c = divmod(at, ld)
    return buf[r:r + klen, c:c + 128] if mode else buf[r:r + 128, c:c + klen]


@pytest.mark.parametrize('c_mode', [R.CM_SET, R.CM_SUB, R.CM_SETNEG])
@pytest.mark.parametrize('a_mode,b_mode', [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_model_is_a_plain_product_on_unflagged_tasks(a_mode, b_mode, c_mode):
    ld, nbatch = 256, 2
    rng = np.random.RandomState(10 + 4 * a_mode + 2 * b_mode + c_mode)
    tasks = [R.task(R.c_tile_off(ld, 0), R.operand_off(ld, k, a_mode, i), R.operand_off(ld, k, b_mode, i + 1), k,
                    R.modes(c_mode, a_mode, b_mode), c_buf=(R.BUF_B, R.BUF_K)[i]) for i, k in enumerate((48, 128))]
    bufs = R.int_bufs(rng, nbatch, ld, tasks)
    out = R.apply_launch(bufs, tasks, R.TS_64x64, R.TG_MISC)
    want = bufs.copy()
    for slot in range(nbatch):
        for t in tasks:
            A = _plain_operand(bufs[slot, t[5]], t[1], t[3], a_mode, ld)
            B = _plain_operand(bufs[slot, t[6]], t[2], t[3], b_mode, ld)
            AB = (A.T if a_mode else A) @ (B if b_mode else B.T)
            C = bufs[slot, t[4], 128:, 128:]
            want[slot, t[4], 128:, 128:] = {R.CM_SET: AB, R.CM_SUB: C - AB, R.CM_SETNEG: -AB}[c_mode]
    assert np.array_equal(out, want)


def test_model_own_pitch():
    ld, ldc = 256, 384
    rng = np.random.RandomState(11)
    tasks = [R.task(R.off(3, 128, ldc), 0, 0, 32, R.modes(R.CM_SUB), c_buf=R.BUF_K)]
    bufs = R.int_bufs(rng, 1, ld, tasks, ldc)
    out = R.apply_launch(bufs, tasks, R.TS_64x64, R.TG_COV, ldc=ldc)
    AB = bufs[0, R.BUF_X, :128, :32] @ bufs[0, R.BUF_KLINV, :128, :32].T
    flat_in, flat_out = bufs[0, R.BUF_K].reshape(-1), out[0, R.BUF_K].reshape(-1)
    for r in range(128):
        at = (3 + r) * ldc + 128
        assert np.array_equal(flat_out[at:at + 128], flat_in[at:at + 128] - AB[r])
    changed = (out != bufs)
    assert changed.sum() <= 128 * 128 and not changed[0, [R.BUF_B, R.BUF_X, R.BUF_KLINV]].any()


@pytest.mark.parametrize('pair', R.PAIRS, ids=R.pair_id)
def test_model_lower_mask(pair):
    """bit 4: 36 of 64 blocks change on the 64 x 64 form of five families; everywhere else every block does"""
    shape, tag = pair
    ld = 256
    rng = np.random.RandomState(12)
    a = R.off(0, 0, ld)
    tasks = [R.task(R.off(128, 128, ld), a, a, 128, R.modes(R.CM_SUB, 0, 0, R.LOWER), R.BUF_B, R.BUF_X, R.BUF_X)]
    bufs = R.int_bufs(rng, 1, ld, tasks)
    bufs[0, R.BUF_X, :128, :128] = 1.0 + np.abs(bufs[0, R.BUF_X, :128, :128])      # A A^T > 0 everywhere
    out = R.apply_launch(bufs, tasks, shape, tag)
    changed = (out != bufs)[0, R.BUF_B, 128:, 128:]
    blocks = changed.reshape(8, 16, 8, 16).all(axis=(1, 3))
    assert np.array_equal(changed.reshape(8, 16, 8, 16).any(axis=(1, 3)), blocks)
    if R.can_lower(shape, tag):
        assert np.array_equal(blocks, np.tril(np.ones((8, 8), dtype=bool))) and blocks.sum() == 36
    else:
        assert blocks.all()
    assert np.array_equal(np.tril(out[0, R.BUF_B, 128:, 128:]),
                          np.tril(bufs[0, R.BUF_B, 128:, 128:] - bufs[0, R.BUF_X, :128, :128] @ bufs[0, R.BUF_X, :128, :128].T))
    assert (~changed | R.may_change(bufs.shape, tasks, shape, tag)[0, R.BUF_B, 128:, 128:]).all()


@pytest.mark.parametrize('n', [256, 232, 129, 128, 1])
def test_model_first_touch_padding(n):
    """the formed tiles are those of B = I + D^1/2 K D^1/2 padded with the identity"""
    ld = 256
    rng = np.random.RandomState(13 + n)
    K = rng.randint(-4, 5, size=(ld, ld)).astype(np.float64)
    s = 2.0 ** rng.randint(-3, 4, size=ld)
    full = np.eye(ld)
    full[:n, :n] += np.outer(s[:n], s[:n]) * K[:n, :n]
    for r0 in (0, 128):
        for c0 in (0, 128):
            assert np.array_equal(R.first_touch_tile(K[r0:r0 + 128, c0:c0 + 128], s, r0, c0, n), full[r0:r0 + 128, c0:c0 + 128])
    # ... and a first-touch task never reads what B held; under bit 4 the quarter above the diagonal keeps it
    a = R.off(0, 0, ld)
    tasks = [R.task(R.off(128, 128, ld), a, a, 32, R.modes(R.CM_SUB, 0, 0, R.LOWER | R.FIRST_TOUCH), R.BUF_B, R.BUF_X, R.BUF_X)]
    bufs = R.int_bufs(rng, 1, ld, tasks)
    bufs[0, R.BUF_K] = K
    bufs[0, R.BUF_B] = R.seeds(rng, (ld, ld))
    out = R.apply_launch(bufs, tasks, R.TS_64x64, R.TG_BULK, ft_s=s[None], ft_n=n)
    A = bufs[0, R.BUF_X, :128, :32]
    want = full[128:, 128:] - A @ A.T
    got = out[0, R.BUF_B, 128:, 128:]
    low = R.block_mask(True)
    assert np.array_equal(got[low], want[low])
    assert R.same_bits(got[:64, 64:], bufs[0, R.BUF_B, 128:192, 192:])
    up_in_quarters = ~low & R.written_mask(True, True)
    assert np.array_equal(got[up_in_quarters], full[128:, 128:][up_in_quarters])


DIAG = [(slice(16 * b, 16 * b + 16), slice(16 * b, 16 * b + 16)) for b in range(8)]


@pytest.mark.parametrize('klen', R.SYM_KLENS)
@pytest.mark.parametrize('pair', R.SYM_FORMS, ids=R.pair_id)
def test_sym_data_tells_the_two_forms_apart(pair, klen):
    """the in-accumulator form (acc = -C, four products at a time) differs from fl(C - A.B) in at least one element of
    EVERY diagonal block of every bit-4 task of the GPU test's launches: a kernel that puts those blocks back into the
    accumulator cannot pass test_sym_accumulates_from_zero"""
    bufs, tasks, ldc = R.sym_case(pair[0], pair[1], klen)
    ld = bufs.shape[2]
    for slot in range(bufs.shape[0]):
        for t in tasks:
            if not t[7] & R.LOWER:
                continue
            A, B = R.operands(bufs, slot, t, ld)
            C = R._window(bufs[slot, t[4]].reshape(-1), t[0], 128, 128, ldc or ld)
            one = R.rounded(R.exact_c_minus_ab(C, A, B))
            many = R.in_accumulator_form(C, A, B)
            assert np.abs(many - one).max() <= (klen // 4 + 1) * 2.0 ** -52      # (the bound the other blocks get)
            for d in DIAG:
                assert (many[d] != one[d]).any()


@pytest.mark.parametrize('table', [1, 0])
def test_sym_chain_data_tells_the_two_forms_apart(table):
    bufs = R.sym_chain_case(table)
    for slot in range(bufs.shape[0]):
        L, C = bufs[slot, R.BUF_B, 128:, :128], bufs[slot, R.BUF_B, 128:, 128:]
        one = R.rounded(R.exact_c_minus_ab(C, L, L.T))
        many = R.in_accumulator_form(C, L, L.T)
        for p in range(8):
            for q in range(p + 1):
                assert (many[16 * p:16 * p + 16, 16 * q:16 * q + 16] != one[16 * p:16 * p + 16, 16 * q:16 * q + 16]).any()


def test_sym_arithmetic_is_exact():
    """S = A.B in float64 equals the integer product whatever the order, and fl(C - S) is what int64 -> float64 rounds to"""
    rng = np.random.RandomState(14)
    A, B, C = R.sym_operand(rng, (128, 512)), R.sym_operand(rng, (512, 128)), R.sym_c(rng, (128, 128))
    S = A @ B
    assert np.array_equal(S, A[:, ::-1] @ B[::-1]) and np.abs(S).max() < 2.0 ** -30
    assert np.array_equal(R.to_units(S), (A * 2.0 ** 28).astype(np.int64) @ (B * 2.0 ** 28).astype(np.int64))
    assert np.array_equal(R.rounded(R.exact_c_minus_ab(C, A, B)), C - S)
    assert (np.frexp(C)[0] * 2.0 ** 53 % 2 == 1).mean() > 0.4             # full mantissas: the last bit is in use


def test_substitution_data_stays_below_2_53():
    L, X = R.unit_lower_pair(np.random.RandomState(3200))
    assert np.array_equal(np.diag(L), np.ones(128)) and np.array_equal(np.triu(L, 1), np.zeros((128, 128)))
    assert set(np.unique(L)) <= {-1.0, 0.0, 1.0} and (np.tril(L, -1) != 0).sum() >= 128
    Li, Xi = L.astype(np.int64).astype(object), X.astype(np.int64).astype(object)
    assert (Li.dot(Xi) == np.eye(128, dtype=np.int64).astype(object)).all()       # exactly, in Python integers
    assert np.array_equal(np.triu(X, 1), np.zeros((128, 128))) and np.array_equal(np.diag(X), np.ones(128))
    # the X part multiplies X_kk by 128-term columns in [-4, 4]; the right-hand sides Y L^T have 128 terms in [-4, 4]
    assert np.abs(X).max() * 4 * 128 < 2.0 ** 53 and 4 * 128 < 2.0 ** 53
    # ... and every intermediate of a substitution is a partial sum of Y L^T: the solve returns Y exactly
    rng = np.random.RandomState(15)
    Y = rng.randint(-4, 5, size=(1, 128, 128)).astype(np.float64)
    bufs = np.zeros((1, 2, 256, 256))
    bufs[0, 0, :128, :128], bufs[0, 1, :128, :128], bufs[0, 0, 128:, :128] = L, X, Y[0] @ L.T
    t = [R.task(R.off(128, 0, 256), R.off(128, 0, 256), 0, 128, R.modes(R.CM_SET), R.BUF_B, R.BUF_B, R.BUF_X)]
    assert np.array_equal(R.apply_panel(bufs, t, 1, acc=True)[0, 0, 128:, :128], Y[0])
