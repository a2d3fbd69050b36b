"""The zero-term predicate in numpy float64, in the kernel's operation order.

exact_dot restates what contrib_of and the shadow-ray derivation compute: dot(hn, normalize(d))
with d = Lpos - hp, dot = x*x' + y*y' + z*z' left to right, normalize = v / sqrt(dot(v, v)) (v
itself when the length is 0), no contraction.  A shadow ray is a zero-term ray when
not (exact_dot > 0) -- a NaN counts, as max(0, NaN) is 0.

certified restates the normalisation-free certificate for shading-time use (the "do not ask for
the ray" stage: built, measured and not merged, DESIGN.md §12.3 and
profiles/r07/stage_b_kernel.patch; kept pinned here for a later attempt): with u = dot(hn, d)
and a = |hn.x d.x| + |hn.y d.y| + |hn.z d.z|, the light is certainly zero-term when
u < -2^-40 a, inside a guarded range of magnitudes.  Why it is sound: the computed u differs from
the exact sum U by at most 3 * 2^-53 a, so U < -(2^-40 - 2^-51) a < 0; normalising scales every
d_k by 1 / |d| with a relative error of a few 2^-53, and the three products and two sums of the
exact dot add a few 2^-53 a / |d| more, far less than |U| / |d| >= 2^-41 a / |d|.  The guard keeps
a, a / |d| and dot(d, d) clear of overflow and of the subnormal range, where those relative
bounds stop holding.  The test checks exactly that claim on adversarial inputs."""
import numpy as np

N = 1 << 18   # per family; eight families, > 10^6 inputs in all


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def normalize(v):
    n = np.sqrt(dot(v, v))
    with np.errstate(all="ignore"):
        return np.where((n > 0.0)[..., None], v / n[..., None], v)


def exact_dot(hn, hp, lpos):
    with np.errstate(all="ignore"):
        return dot(hn, normalize(lpos - hp))


def certified(hn, hp, lpos):
    with np.errstate(all="ignore"):
        d = lpos - hp
        u = dot(hn, d)
        a = np.abs(hn[..., 0] * d[..., 0]) + np.abs(hn[..., 1] * d[..., 1]) + np.abs(hn[..., 2] * d[..., 2])
        dmax = np.abs(d).max(-1)
        guard = (dmax >= 2.0 ** -200) & (dmax <= 2.0 ** 200) & (a >= 2.0 ** -400) & (a <= 2.0 ** 400)
        return guard & (u < -(2.0 ** -40) * a)


def families(rng):
    hn = rng.normal(size=(N, 3))
    hp = rng.normal(size=(N, 3)) * 3.0
    lp = rng.normal(size=(N, 3)) * 5.0
    yield "random", hn, hp, lp
    # dots within a few ulps of zero: d made orthogonal to hn, then nudged by 0..4 ulps per component
    d = lp - hp
    d = d - hn * (dot(hn, d) / dot(hn, hn))[:, None]
    for _ in range(4):
        d = np.where(rng.random((N, 3)) < 0.5, np.nextafter(d, np.inf), np.nextafter(d, -np.inf))
    yield "near_zero", hn, np.zeros((N, 3)), d
    # axis-aligned normals, lights in and next to the surface's plane
    ax = np.eye(3)[rng.integers(0, 3, N)] * rng.choice([-1.0, 1.0], N)[:, None]
    lp2 = lp.copy()
    k = np.argmax(np.abs(ax), -1)
    off = rng.choice([0.0, 1e-9, -1e-9, 1e-300, -1e-300, 5e-324, -5e-324], N)
    lp2[np.arange(N), k] = hp[np.arange(N), k] + off
    yield "axis_in_plane", ax, hp, lp2
    yield "axis_random", ax, hp, lp
    # components spanning 2^+-150 (products reach 2^+-300: over the guard on both sides)
    s1 = 2.0 ** rng.integers(-150, 151, (N, 3))
    s2 = 2.0 ** rng.integers(-150, 151, (N, 3))
    yield "wide_range", hn * s1, np.zeros((N, 3)), lp * s2
    yield "wide_near_zero", hn * s1, np.zeros((N, 3)), d * s2
    # extreme magnitudes: overflow of dot(d, d), subnormal products
    s3 = 2.0 ** rng.integers(-1070, 1020, (N, 1))
    yield "extreme", hn, np.zeros((N, 3)), lp * s3
    # d = 0 (light at the shading point) and non-finite normals
    hn_bad = hn.copy()
    hn_bad[::3, 0] = np.nan
    hn_bad[1::3, 1] = np.inf
    yield "degenerate", hn_bad, hp, np.where((np.arange(N) % 2 == 0)[:, None], hp, lp)


def test_certificate_never_fires_on_a_light_in_front():
    rng = np.random.default_rng(20240607)
    total = 0
    for name, hn, hp, lp in families(rng):
        c = certified(hn, hp, lp)
        e = exact_dot(hn, hp, lp)
        bad = c & (e > 0.0)
        assert not bad.any(), (name, int(bad.sum()))
        total += len(c)
    assert total >= 10 ** 6


def test_certificate_fires_on_ordinary_back_facing_inputs():
    rng = np.random.default_rng(7)
    hn = rng.normal(size=(N, 3))
    hp = rng.normal(size=(N, 3)) * 3.0
    lp = rng.normal(size=(N, 3)) * 5.0
    e = exact_dot(hn, hp, lp)
    back = e < -1e-6 * np.sqrt(dot(hn, hn))
    assert back.sum() > N // 3
    assert certified(hn, hp, lp)[back].all()
    assert not certified(hn, hp, lp)[e > 0.0].any()


def test_exact_predicate_counts_nan_and_zero():
    hn = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [np.nan, 1.0, 0.0], [0.0, 1.0, 0.0]])
    hp = np.zeros((4, 3))
    lp = np.array([[5.0, 0.0, 0.3], [1.0, -2.0, 0.0], [0.0, 3.0, 0.0], [0.0, 3.0, 0.0]])
    e = exact_dot(hn, hp, lp)
    assert list(~(e > 0.0)) == [True, True, True, False]   # in plane, behind, NaN normal, in front
