"""Each HIP kernel family on its own against NumPy (through the C ABI's
diagnostic entry points).  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

from gpyrn_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _hip.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('a_mode,b_mode', [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize('c_mode', [0, 1, 2])
def test_tile_gemm_layouts(ctx, a_mode, b_mode, c_mode):
    # asymmetric integer data: any row/col or operand-order swap shows up exactly
    rng = np.random.RandomState(5 + 4 * a_mode + 2 * b_mode + c_mode)
    M, N, K = 256, 128, 48
    A = rng.randint(-4, 5, size=(M, K)).astype(float)
    B = rng.randint(-4, 5, size=(K, N)).astype(float)
    C0 = rng.randint(-9, 10, size=(M, N)).astype(float)
    out = ctx.test_gemm(A, B, C0, a_mode, b_mode, c_mode)
    want = {0: A @ B, 1: C0 - A @ B, 2: -(A @ B)}[c_mode]
    assert np.array_equal(out, want)


@pytest.mark.parametrize('shape', [1, 2, 3])
@pytest.mark.parametrize('a_mode,b_mode', [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_tile_gemm_small_workgroup_shapes(ctx, shape, a_mode, b_mode):
    # the 64x64 / 64x128 / 128x64 cuts of a 128x128 task (latency-bound launches)
    rng = np.random.RandomState(50 + 16 * shape + 4 * a_mode + 2 * b_mode)
    M, N, K = 256, 384, 80
    A = rng.randint(-4, 5, size=(M, K)).astype(float)
    B = rng.randint(-4, 5, size=(K, N)).astype(float)
    C0 = rng.randint(-9, 10, size=(M, N)).astype(float)
    out = ctx.test_gemm(A, B, C0, a_mode, b_mode, 1 | (shape << 4))
    assert np.array_equal(out, C0 - A @ B)


def test_tile_gemm_random_fp64(ctx):
    rng = np.random.RandomState(1)
    A = rng.standard_normal((384, 512))
    B = rng.standard_normal((512, 256))
    C0 = rng.standard_normal((384, 256))
    out = ctx.test_gemm(A, B, C0, 0, 0, 1)
    np.testing.assert_allclose(out, C0 - A @ B, rtol=0, atol=5e-12)


def _spd(n, rng, cond_shift=1.0):
    t = np.sort(rng.uniform(0, 0.4 * n, n))
    r = t[:, None] - t[None, :]
    return np.exp(-0.5 * r**2 / 30.0**2) * np.outer(1 + rng.rand(n), 1 + rng.rand(n)) ** 0 \
        + cond_shift * np.eye(n)


# (384, 18): more matrices than the chain's kernels take pointers for as kernel arguments (GPRN_ARG_SLOTS = 16): their
# pointer-table forms run
@pytest.mark.parametrize('n,batch', [(128, 1), (256, 2), (640, 3), (384, 18)])
def test_factor_invert(ctx, n, batch):
    rng = np.random.RandomState(n)
    A = np.array([_spd(n, rng, 1.0 + b) for b in range(batch)])
    L, X, info = ctx.test_factor_invert(A)
    assert info == 0
    for b in range(batch):
        Lref = np.linalg.cholesky(A[b])
        np.testing.assert_allclose(L[b], Lref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.tril(X[b]), np.linalg.inv(Lref), rtol=0, atol=1e-11)
        # diagonal tiles of X carry explicit zeros above the diagonal
        for k in range(n // 128):
            blk = X[b][k * 128:(k + 1) * 128, k * 128:(k + 1) * 128]
            assert np.array_equal(np.triu(blk, 1), np.zeros_like(blk))
        np.testing.assert_allclose(np.tril(X[b]) @ Lref, np.eye(n), rtol=0, atol=1e-11)


def test_factor_invert_not_positive_definite(ctx):
    rng = np.random.RandomState(3)
    A = _spd(256, rng)
    A[200, 200] = -1.0
    L, X, info = ctx.test_factor_invert(A)
    assert info == 201                         # LAPACK-style order of the failing minor
    assert np.isnan(L[0][255, 255])            # jax semantics: NaN, no exception


@pytest.mark.parametrize('n,batch,flags', [(128, 1, 1), (384, 3, 1), (384, 18, 1), (384, 50, 1), (1024, 5, 1), (1024, 5, 0)])
def test_factor_invert_with_substitution_panels(ctx, n, batch, flags):
    """Round 6: the factorisation of a PRIOR matrix solves its panel steps instead of multiplying by explicit inverses of
    diagonal blocks (csrc/diag_tile.h ACC: base16_regs<true>, subst16_row, trsm_rows16; option accurate_factor).  Here on its
    own, in every launch form -- pointers as kernel arguments or from the table (batch > 16), the chain's products on the
    latency kernels or as tile tasks (batch >= 48), latency and throughput task lists (batch x tiles > 32: outer panels with
    K = 512 updates), flags and events -- on a pure Periodic kernel under the reference's nugget (cond(K) ~ 1e8-1e9) with a
    vector far outside its range: |X m|^2 agrees with LAPACK's cholesky + triangular solve to 2e-9 (each is a few 1e-10
    from a long-double evaluation: profiles/r06_prior_term_accuracy.txt), where the product form is 1e-8 ... 1e-7 away."""
    from scipy.linalg import solve_triangular
    from gpyrn_amd import covfunc
    if flags and not ctx.option('flags'):
        pytest.skip('device-side flags are off for this context')
    rng = np.random.RandomState(n + batch)
    N = n - 24                                             # (a ragged last tile: identity padding)
    t = np.sort(rng.uniform(0.0, 0.8 * N, N))
    K = covfunc.Periodic(1.34, 22.7, 0.82)(t[:, None] - t[None, :]) + 1e-6 * np.eye(N)
    A = np.eye(n)
    A[:N, :N] = K
    m = 10.0 * rng.standard_normal(N)
    a = solve_triangular(np.linalg.cholesky(K), m, lower=True)
    want = float(a @ a)
    old_flags, devs = ctx.option('flags', flags), {}
    try:
        for acc in (1, 0):
            ctx.option('accurate_factor', acc)
            L, X, info = ctx.test_factor_invert(np.array([A] * batch))
            assert info == 0
            got = [float(np.sum((np.tril(X[b])[:N, :N] @ m) ** 2)) for b in range(batch)]
            assert len(set(got)) == 1, 'the copies of one matrix in a batch differ'
            devs[acc] = abs(got[0] - want) / want
            if acc:
                np.testing.assert_allclose(np.tril(L[0])[:N, :N] @ np.tril(L[0])[:N, :N].T, K, rtol=0, atol=1e-12 * np.abs(K).max())
    finally:
        ctx.option('accurate_factor', -2)
        ctx.option('flags', old_flags)
    assert devs[1] <= 2e-9, devs
    assert devs[0] >= 5 * devs[1], 'the product form was expected to be visibly worse on this matrix: %r' % devs
    assert ctx.option('fallbacks') == 0


def test_lauum(ctx):
    rng = np.random.RandomState(9)
    X = np.tril(rng.standard_normal((384, 384)))
    out = ctx.test_lauum(X)
    np.testing.assert_allclose(np.tril(out), np.tril(X.T @ X), rtol=0, atol=1e-11)


@pytest.mark.parametrize('n', [128, 256, 640, 1152])
def test_lauum_sizes(ctx, n):
    # one tile, an even count, an odd count, more tiles than an outer panel (the K = 512 lists run); integer data: every
    # partial sum is representable, so the lower triangle is X^T X exactly, in any summation order
    rng = np.random.RandomState(90 + n)
    X = np.tril(rng.randint(-3, 4, size=(n, n))).astype(float)
    out = ctx.test_lauum(X)
    assert np.array_equal(np.tril(out), np.tril(X.T @ X))
    X = np.tril(rng.standard_normal((n, n)))
    out = ctx.test_lauum(X)
    np.testing.assert_allclose(np.tril(out), np.tril(X.T @ X), rtol=0, atol=1e-11)


def _check_factor_by_probes(A, L, X, rng, tol):
    """O(n^2) checks of a factor + inverse: L L^T v = A v and X (L v) = v for random v."""
    n = A.shape[0]
    v = rng.standard_normal((n, 3))
    Lt = np.tril(L)
    np.testing.assert_allclose(Lt @ (Lt.T @ v), A @ v, rtol=0, atol=tol * np.abs(A @ v).max())
    np.testing.assert_allclose(np.tril(X) @ (Lt @ v), v, rtol=0, atol=tol * np.abs(v).max())


@pytest.mark.parametrize('flags', [0, 1])
def test_factor_invert_schedules_at_size(ctx, flags):
    # the HIP-event schedule lost a dependency that only shows with many tile steps
    # and a batch that keeps stream3 behind the chain: N = 4096 (32 tile steps), 8 matrices.
    can_flags = ctx.option('flags')
    if flags and not can_flags:
        pytest.skip('device-side flags are off for this context (serialising tool or no stream memory ops)')
    old = ctx.option('flags', flags)
    try:
        rng = np.random.RandomState(77)
        n, batch = 4096, 8
        A = np.array([_spd(n, rng, 1.0 + 0.25 * b) for b in range(batch)])
        L, X, info = ctx.test_factor_invert(A)
        assert info == 0
        for b in range(batch):
            Lref = np.linalg.cholesky(A[b])
            np.testing.assert_allclose(np.tril(L[b]), Lref, rtol=0, atol=2e-11)
            _check_factor_by_probes(A[b], L[b], X[b], rng, 1e-10)
    finally:
        ctx.option('flags', old)


def test_factor_invert_flag_schedule_t128(ctx):
    # the default (flag) schedule at BASELINE config 5's matrix size, T = 128 tile steps, with more than two
    # matrices -- the un-split "rest" path of factor_invert_split (T > 64) and launches of thousands of workgroups.  In
    # round 3 the last tile step's panel launch polled in-kernel in every one of its 2 (T - 1) x batch workgroups, filled
    # the device and kept its own producer off the CUs: the wait ran into its budget and the call was silently re-run on
    # HIP events.  The factors are checked as always; what this test adds is that NO fallback happened.
    if not ctx.option('flags'):
        pytest.skip('device-side flags are off for this context (serialising tool or no stream memory ops)')
    rng = np.random.RandomState(83)
    n, batch = 16384, 3
    A = np.array([_spd(n, rng, 1.5 + 0.5 * b) for b in range(batch)])
    before = ctx.option('fallbacks')
    L, X, info = ctx.test_factor_invert(A)
    assert info == 0
    assert ctx.option('fallbacks') == before and ctx.option('flags') == 1
    for b in range(batch):
        _check_factor_by_probes(A[b], L[b], X[b], rng, 1e-9)
        d = np.diag(L[b])
        assert np.all(d > 0) and np.isfinite(d).all()


def test_factor_invert_event_schedule_n16384(ctx):
    # once, at BASELINE config 5's matrix size (128 tile steps), on the event schedule
    old = ctx.option('flags', 0)
    try:
        rng = np.random.RandomState(78)
        n = 16384
        A = _spd(n, rng, 1.5)
        L, X, info = ctx.test_factor_invert(A)
        assert info == 0
        _check_factor_by_probes(A, L[0], X[0], rng, 1e-9)
        d = np.diag(L[0])
        assert np.all(d > 0) and np.isfinite(d).all()
    finally:
        ctx.option('flags', old)


def test_wait_timeout_falls_back_to_events(ctx, capfd):
    # A producer flag that never goes up (test hook) makes an in-kernel wait give up after the budget;
    # the call is then re-run on HIP events: correct numbers, one warning, flags latched off.
    if not ctx.option('flags'):
        pytest.skip('device-side flags are off for this context')
    rng = np.random.RandomState(79)
    n = 1024
    A = np.array([_spd(n, rng, 1.0), _spd(n, rng, 2.0)])
    before = ctx.option('fallbacks')
    ctx.option('wait_budget_ms', 20)
    ctx.option('withhold_inner', 2)
    try:
        L, X, info = ctx.test_factor_invert(A)
    finally:
        ctx.option('withhold_inner', 0)
        ctx.option('wait_budget_ms', 2000)
    assert info == 0
    for b in range(2):
        np.testing.assert_allclose(np.tril(L[b]), np.linalg.cholesky(A[b]), rtol=0, atol=1e-11)
        _check_factor_by_probes(A[b], L[b], X[b], rng, 1e-10)
    assert ctx.option('fallbacks') == before + 1
    assert ctx.option('flags') == 0                      # latched for the context
    assert 'timed out' in capfd.readouterr().err
    # the next call runs on events straight away, no new fallback
    L2, X2, info = ctx.test_factor_invert(A)
    assert info == 0 and ctx.option('fallbacks') == before + 1
    np.testing.assert_array_equal(L2, L)
    ctx.option('flags', 1)                               # the module fixture goes on with flags


def test_oversized_lds_pad_is_an_error_not_an_abort(ctx):
    # VERDICT r2 #4 (gpurun_out/r2_b37.err): an LDS pad that does not fit on top of a tile kernel's static image
    # used to reach the queue and abort the process (HSA_STATUS_ERROR_INVALID_ALLOCATION).  Every launch that
    # carries a pad is now checked against the device's LDS per workgroup: GPRN_E_ARG with text, the shared streams
    # drained, and the context good for the next call.
    _oversized_pad(ctx)


def _oversized_pad(ctx):
    rng = np.random.RandomState(81)
    n, batch = 2048, 3                                   # three matrices: the bulk launches take "bulk_pad_kb"
    A = np.array([_spd(n, rng, 1.0 + 0.5 * b) for b in range(batch)])
    ctx.option('bulk_pad_kb', 400)
    try:
        with pytest.raises(_hip.BackendError, match='LDS'):
            ctx.test_factor_invert(A)
    finally:
        ctx.option('bulk_pad_kb', -2)                    # back to the default
    before = ctx.option('fallbacks')
    L, X, info = ctx.test_factor_invert(A)
    assert info == 0 and ctx.option('fallbacks') == before
    for b in range(batch):
        np.testing.assert_allclose(np.tril(L[b]), np.linalg.cholesky(A[b]), rtol=0, atol=2e-11)
    # a pad that fits is just a pad
    ctx.option('bulk_pad_kb', 24)
    try:
        L2, _, info = ctx.test_factor_invert(A)
    finally:
        ctx.option('bulk_pad_kb', -2)
    assert info == 0
    np.testing.assert_array_equal(L2, L)


def test_live_contexts_share_the_device_streams():
    # Contexts of one process share ONE set of streams per device: with four streams per context the runtime
    # put the second context's chain and side streams on the same hardware queue and every flag-schedule call
    # on it ran into the wait budget (r2 finding).  Four live contexts, used in turn: right numbers, no fallback,
    # still on flags.
    rng = np.random.RandomState(80)
    n = 1024
    A = _spd(n, rng, 1.0)
    live = [_hip.Context(0) for _ in range(4)]
    try:
        can_flags = live[0].option('flags')
        Ls = []
        for _ in range(2):
            for c in live:
                L, X, info = c.test_factor_invert(A)
                assert info == 0
                Ls.append(L)
        for L in Ls[1:]:
            np.testing.assert_array_equal(L, Ls[0])
        np.testing.assert_allclose(np.tril(Ls[0][0]), np.linalg.cholesky(A), rtol=0, atol=1e-11)
        assert [c.option('fallbacks') for c in live] == [0] * 4
        assert [c.option('flags') for c in live] == [can_flags] * 4
    finally:
        for c in live:
            c.close()
