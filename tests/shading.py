"""Restatement of the fragment stage (include/ocean_consumers.h: ocean_sky_coefficients, ocean_sky_radiance, ocean_eval_seabed,
ocean_shade_points) for the tests, written from the reference's shader text (SkyPreetham.cpp, SkyPreetham.frag, WaterSurfaceMesh.frag).

Two parts.

1. The seabed noise in float32 numpy, step for step as the header orders it: the device is held to it in every bit.

2. The optics, evaluated once in float64 on the fp32 inputs, with a running error: every value is a `Num` (value, error).  The error is
   the first-order bound of what an fp32 evaluation of the same formulas may be off by:
     * every rounded operation adds 2^-24 |v| + 2^-126 (the second term is fp32 underflow);
     * every transcendental (exp, pow, acos, sin, cos, tan) adds 4 * 2^-24 |v|: a few ulps each, what a full-precision device library gives;
     * a univariate function g propagates max |g(x +- e) - g(x)|, evaluated, not differentiated -- finite at acos(1), across the smoothstep
       edge (slope 333), through pow with exponents 32 .. 512 and across the pole of tan;
     * products and quotients propagate by |a| eb + |b| ea (+ ea eb) and (ea + |q| eb) / (|b| - eb);
     * the shader's literals (0.05f, 1e-3f, 0.997f, the matrix) are fp32 numbers and exact; constants the host derives and rounds once
       (1/ior, pi, 0.1 absorb, 0.33 backscatter / absorb, the normal-incidence reflectance) carry 2^-24 |c|.
   The same code evaluates the formulas in float32 (dtype=np.float32): tests/test_shading.py shows that evaluation stays under the bound.
   A point is AMBIGUOUS where the reference Fresnel branch theta_i <= 1e-5 could go either way within the error of theta_i.
   The seabed's (normal, factor) is an input: the noise is never evaluated in float64 (hash1 resolves 2^-7 at its largest arguments).
   `mut` selects one deliberate mistake, for the tests that show the bound has teeth."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
IOR = 1.33477
MUTATIONS = ("transpose", "no_disk", "no_kbias", "fresnel_swap", "dy_for_dot", "no_depth", "raised_ray")


# ---- 1. seabed noise, float32 -----------------------------------------------------------------------------------------------------------------
INV_PI_F = f32(0.31830987)


def _fract(a):
    return a - np.floor(a)


def hash1(ix, iy):
    jx = f32(50.0) * _fract(ix * INV_PI_F)
    jy = f32(50.0) * _fract(iy * INV_PI_F)
    return _fract((jx * jy) * (jx + jy))


def noise(px, py):
    ix, iy = np.floor(px), np.floor(py)
    fx, fy = px - ix, py - iy
    ux = ((fx * fx) * fx) * (fx * (fx * f32(6.0) - f32(15.0)) + f32(10.0))
    uy = ((fy * fy) * fy) * (fy * (fy * f32(6.0) - f32(15.0)) + f32(10.0))
    one = f32(1.0)
    a, b, c, d = hash1(ix, iy), hash1(ix + one, iy), hash1(ix, iy + one), hash1(ix + one, iy + one)
    return f32(-1.0) + f32(2.0) * (((a + (b - a) * ux) + (c - a) * uy) + ((((a - b) - c) + d) * ux) * uy)


def fbm4(px, py):
    v, g = np.zeros_like(px), f32(0.5)
    for _ in range(4):
        v = v + g * noise(px, py)
        g = g * f32(0.5)
        px, py = f32(1.6) * px + f32(1.2) * py, f32(-1.2) * px + f32(1.6) * py
    return v


def seabed_height(x, z):
    return f32(0.0) - f32(8.0) * fbm4(z * f32(0.02), x * f32(0.02))


def seabed(xz):
    """(n.x, n.y, n.z, colour factor) at terrain points xz [count, 2]: float32 in, float32 out, every step rounded as the device rounds it."""
    xz = np.ascontiguousarray(xz, dtype=f32).reshape(-1, 2)
    x, z = xz[:, 0].copy(), xz[:, 1].copy()
    with np.errstate(all="ignore"):
        factor = np.minimum(np.maximum(fbm4((z * f32(0.02)) * f32(2.0), (x * f32(0.02)) * f32(2.0)), f32(0.6)), f32(0.9))
        e = f32(1e-4)
        nx = seabed_height(x - e, z) - seabed_height(x + e, z)
        ny = np.full_like(x, f32(10.0) * e)
        nz = seabed_height(x, z - e) - seabed_height(x, z + e)
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        out = np.stack([nx / ln, ny / ln, nz / ln, factor], axis=1)
    assert out.dtype == f32
    return out


# ---- 2. optics: values with a running error -----------------------------------------------------------------------------------------------------
class Num:
    """An array of values (float64 for the restatement, float32 for the plain evaluation) with the running fp32 error bound of each."""
    __slots__ = ("v", "e")
    __array_ufunc__ = None

    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros(np.shape(v)) if e is None else e

    def _lift(self, o):
        if isinstance(o, Num):
            return o
        return Num(np.full_like(self.v, self.v.dtype.type(f32(o))))         # a literal of the shader: an fp32 number, exact

    def _rounded(self, v, e):
        return Num(v, e + U * np.abs(v.astype(np.float64)) + TINY)

    def __add__(self, o):
        o = self._lift(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = self._lift(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = self._lift(o)
        a, b = np.abs(self.v.astype(np.float64)), np.abs(o.v.astype(np.float64))
        return self._rounded(self.v * o.v, a * o.e + b * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = self._lift(o)
        q = self.v / o.v
        den = np.abs(o.v.astype(np.float64)) - o.e
        e = np.where(den > 0.0, (self.e + np.abs(q.astype(np.float64)) * o.e) / np.where(den > 0.0, den, 1.0), np.inf)
        return self._rounded(q, e)

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return self._lift(o) - self

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def __neg__(self):
        return Num(-self.v, self.e)

    def fn(self, g, lo=-np.inf, hi=np.inf, ulps=4):
        """g applied to the values; the error is what g does to x +- e (kept inside [lo, hi]) plus `ulps` of its own."""
        x = self.v.astype(np.float64)
        g0 = g(x)
        spread = np.maximum(np.abs(g(np.clip(x + self.e, lo, hi)) - g0), np.abs(g(np.clip(x - self.e, lo, hi)) - g0))
        spread = np.where(np.isfinite(spread), spread, np.inf)
        v = g(self.v).astype(self.v.dtype)
        return Num(v, spread + ulps * U * np.abs(g0) + TINY)

    def clamp(self, lo, hi):
        return Num(np.minimum(np.maximum(self.v, self.v.dtype.type(lo)), self.v.dtype.type(hi)), self.e)

    def abs(self):
        return Num(np.abs(self.v), self.e)


def const(like, value, rel=U):
    """A launch-uniform constant the device rounds to fp32 once (rel = its relative error; 0 for an fp32 input)."""
    value = float(value)
    return Num(np.full_like(like.v, like.v.dtype.type(value)), np.full(like.v.shape, rel * abs(value)))


def where(cond, a, b):
    return Num(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normalize3(a):
    ln = dot3(a, a).fn(np.sqrt, lo=0.0, ulps=1)
    return [a[0] / ln, a[1] / ln, a[2] / ln]


def sky_coefficients(turbidity, sun_dir):
    """SkyPreetham::Update in float64 on the fp32 inputs, each output rounded to fp32 once: the header's text.  Returns a dict of float32
    arrays: sun [3], A, B, C, D, E, zenith, zero [3] each, and turbidity."""
    t = float(f32(turbidity))
    s = np.asarray(sun_dir, dtype=f32).astype(np.float64)
    s = s / np.sqrt((s * s).sum())
    th = np.arccos(max(s[1], 0.0))
    A = np.array([0.1787 * t - 1.4630, -0.0193 * t - 0.2592, -0.0167 * t - 0.2608])
    B = np.array([-0.3554 * t + 0.4275, -0.0665 * t + 0.0008, -0.0950 * t + 0.0092])
    C = np.array([-0.0227 * t + 5.3251, -0.0004 * t + 0.2125, -0.0079 * t + 0.2102])
    D = np.array([0.1206 * t - 2.5771, -0.0641 * t - 0.8989, -0.0441 * t - 1.6537])
    E = np.array([-0.0670 * t + 0.3703, -0.0033 * t + 0.0452, -0.0109 * t + 0.0529])
    chi = (4.0 / 9.0 - t / 120.0) * (np.pi - 2.0 * th)
    th2, th3, t2 = th * th, th * th * th, t * t
    zen = np.array([
        (4.0453 * t - 4.9710) * np.tan(chi) - 0.2155 * t + 2.4192,
        (0.00165 * th3 - 0.00375 * th2 + 0.00209 * th) * t2 + (-0.02903 * th3 + 0.06377 * th2 - 0.03202 * th + 0.00394) * t
        + (0.11693 * th3 - 0.21196 * th2 + 0.06052 * th + 0.25886),
        (0.00275 * th3 - 0.00610 * th2 + 0.00317 * th) * t2 + (-0.04214 * th3 + 0.08970 * th2 - 0.04153 * th + 0.00516) * t
        + (0.15346 * th3 - 0.26756 * th2 + 0.06670 * th + 0.26688)])
    zero = (1.0 + A * np.exp(B / np.cos(0.0))) * (1.0 + C * np.exp(D * th) + E * np.cos(th) ** 2)
    return dict(sun=s.astype(f32), turbidity=f32(t), A=A.astype(f32), B=B.astype(f32), C=C.astype(f32), D=D.astype(f32), E=E.astype(f32),
                zenith=zen.astype(f32), zero=zero.astype(f32))


def coefficients_of(k):
    """The same dict from the library's struct ocean_sky_coeffs (watersurfacerendering_amd.sky_coefficients)."""
    g = lambda a: np.array(list(a)[:3], dtype=f32)
    return dict(sun=g(k.sun_dir), turbidity=f32(k.turbidity), A=g(k.A), B=g(k.B), C=g(k.C), D=g(k.D), E=g(k.E), zenith=g(k.zenith_lum),
                zero=g(k.zero_theta_sun))


RGB_M = ((2.3706743, -0.9000405, -0.4706338), (-0.5138850, 1.4253036, 0.0885814), (0.0052982, -0.0146949, 1.0093968))


def sky_lum(co, d, mut=None):
    """SKY(d) of the header for a direction d (three Num) taken as it is: (L [3], disk, Yxy [3])."""
    one = d[0]
    inp = lambda x: const(one, x, 0.0)                      # an fp32 input: exact
    sun = [inp(co["sun"][k]) for k in range(3)]
    cy = d[1].clamp(0.0, 1.0)
    cg = (cy if mut == "dy_for_dot" else dot3(sun, d).clamp(0.0, 1.0))
    theta, gamma = cy.fn(np.arccos, -1.0, 1.0), cg.fn(np.arccos, -1.0, 1.0)
    ct = theta.fn(np.cos)
    if mut != "no_kbias":
        ct = ct + 1e-3
    cgm = gamma.fn(np.cos)
    yxy = []
    for k in range(3):
        A, B, C, D, E = (inp(co[n][k]) for n in "ABCDE")
        f = (1.0 + A * (B / ct).fn(np.exp)) * ((1.0 + C * (D * gamma).fn(np.exp)) + (E * cgm) * cgm)
        yxy.append(inp(co["zenith"][k]) * (f / inp(co["zero"][k])))
    yy = yxy[0] / yxy[2]
    xyz = [yxy[1] * yy, yxy[0], ((1.0 - yxy[1]) - yxy[2]) * yy]
    m = RGB_M if mut != "transpose" else tuple(zip(*RGB_M))
    L = [(m[k][0] * xyz[0] + m[k][1] * xyz[1]) + m[k][2] * xyz[2] for k in range(3)]
    s = ((cg - 0.997) / const(one, float(f32(1.0) - f32(0.997)), 0.0)).clamp(0.0, 1.0)
    disk = (s * s) * (3.0 - 2.0 * s)
    if mut == "no_disk":
        disk = inp(0.0)
    return L, disk, yxy


def _columns(a, dtype):
    a = np.ascontiguousarray(a, dtype=f32)
    return [Num(a[:, k].astype(dtype)) for k in range(a.shape[1])]


def sky_radiance(co, sun_color, dirs, dtype=np.float64, mut=None):
    """ocean_sky_radiance restated: (values [count, 4], bound [count, 4]) for directions dirs [count, 3] (float32)."""
    with np.errstate(all="ignore"):
        d = normalize3(_columns(np.asarray(dirs, dtype=f32).reshape(-1, 3), dtype))
        L, disk, _ = sky_lum(co, d, mut)
        out = [L[k] * 0.05 + (const(disk, sun_color[k], 0.0) * disk) * L[k] for k in range(3)] + [disk]
    return np.stack([o.v for o in out], axis=1), np.stack([o.e for o in out], axis=1)


def water_dict(w):
    """The fields of a struct ocean_water as float32 numpy values."""
    out = {}
    for name, kind in w._fields_:
        v = getattr(w, name)
        out[name] = np.array(list(v), dtype=f32) if hasattr(v, "__len__") else (int(v) if isinstance(v, int) else f32(v))
    return out


def shade(co, sky, water, pos, nrm, seabed_rows=None, dtype=np.float64, mut=None):
    """ocean_shade_points restated.  co: the coefficient dict; sky: dict(sun_color [3], sun_intensity); water: water_dict(...);
    pos, nrm [count, 4] float32; seabed_rows [count, 4]: the (normal, factor) to use at each point's p_g (None: the FLAT seabed of `water`).
    Returns dict(rgba, rgba_bound, aux, aux_bound [count, 4], ambiguous [count]), tone-mapped where water['tonemap']."""
    with np.errstate(all="ignore"):
        px, py, pz, pw = _columns(pos, dtype)
        n = normalize3(_columns(np.asarray(nrm, dtype=f32)[:, :3], dtype))
        one = px
        inp = lambda x: const(one, x, 0.0)
        cam = [inp(water["cam_pos"][k]) for k in range(3)]
        sun = [inp(co["sun"][k]) for k in range(3)]
        pwy = py + inp(water["height"])
        target = [px, pwy if mut == "raised_ray" else py, pz]
        d = normalize3([target[k] - cam[k] for k in range(3)])
        dn = dot3(n, d)
        k2 = 2.0 * dn
        L, disk, _ = sky_lum(co, [d[k] - k2 * n[k] for k in range(3)], mut)
        S = [L[k] * 0.05 + disk * L[k] for k in range(3)]
        ndl = dot3(n, sun).clamp(0.0, np.inf)
        ka = inp(water["sky_intensity"]) * ndl
        hw = normalize3([sun[k] - d[k] for k in range(3)])
        ndh = dot3(n, hw).clamp(0.0, np.inf)
        h = float(water["specular_highlights"])
        spec = inp(water["specular_intensity"]) * ndh.fn(lambda x: np.power(x, h), lo=0.0).clamp(0.0, 1.0)
        ks = inp(sky["sun_intensity"]) * spec
        eta = const(one, 1.0 / IOR)
        c = -dot3(n, sun)
        kk = 1.0 - (eta * eta) * (1.0 - c * c)
        m = eta * c + kk.fn(np.sqrt, lo=0.0, ulps=1)
        refr = [where(kk.v >= 0, -(eta * sun[k]) - m * n[k], inp(0.0)) for k in range(3)]
        tg = -(pwy / refr[1])
        g = [px + tg * refr[0], pwy + tg * refr[1], pz + tg * refr[2]]
        if seabed_rows is None:
            ng, factor = [inp(0.0), inp(1.0), inp(0.0)], inp(water["seabed_factor"])
        else:
            sb = _columns(seabed_rows, dtype)
            ng, factor = sb[:3], sb[3]
        lg = factor * -dot3(ng, refr)
        depth = (pwy - g[1]).abs()
        ci = -dn
        if int(water["fresnel"]) == 1:
            ior = const(one, IOR)
            ct = (1.0 - (1.0 - ci * ci) / (ior * ior)).fn(np.sqrt, lo=0.0, ulps=1)
            rs, rp = (ci - ior * ct) / (ci + ior * ct), (ior * ci - ct) / (ior * ci + ct)
            fr = where(ci.v > 0, 0.5 * (rs * rs + rp * rp), inp(1.0))
            ambiguous = np.zeros(ci.v.shape, dtype=bool)
        else:
            tt = -dot3(n, refr)
            ti, tu = (tt, ci) if mut == "fresnel_swap" else (ci, tt)
            t1 = (ti - tu).fn(np.sin) / (ti + tu).fn(np.sin)
            t2 = (ti - tu).fn(np.tan) / (ti + tu).fn(np.tan)
            f0 = const(one, ((IOR - 1.0) / (IOR + 1.0)) ** 2)
            fr = where(ti.v <= ti.v.dtype.type(1e-5), f0, 0.5 * (t1 * t1 + t2 * t2))
            ambiguous = np.abs(ti.v.astype(np.float64) - float(f32(1e-5))) <= ti.e
        col = []
        for k in range(3):
            la, ls = ka * S[k], ks * S[k]
            a01, s01 = const(one, float(water["absorb"][k]) * 0.1), const(one, float(water["scatter"][k]) * 0.1)
            df0 = const(one, 0.33 * float(water["backscatter"][k]) / float(water["absorb"][k]))
            ldf0 = df0 * ((const(one, np.pi) * la) * const(one, 1.0 / np.pi))
            att0 = (-(a01 * tg)).fn(np.exp)
            att1 = att0 if mut == "no_depth" else (-(a01 * tg) - s01 * depth).fn(np.exp)
            lu = att0 * (lg * inp(water["terrain_color"][k])) + (1.0 - att1) * ldf0
            col.append(fr * (ls + la) + (1.0 - fr) * lu)
        if int(water["foam_white"]):
            col = [where(pw.v < 0, inp(1.0), x) for x in col]
        col.append(inp(1.0))
        if int(water["tonemap"]):
            col = [1.0 - (-2.0 * x).fn(np.exp) for x in col]
        aux = [g[0], g[2], tg, fr]
    st = lambda xs, what: np.stack([getattr(x, what) for x in xs], axis=1)
    return dict(rgba=st(col, "v"), rgba_bound=st(col, "e"), aux=st(aux, "v"), aux_bound=st(aux, "e"), ambiguous=ambiguous)


# ---- the inputs the GPU tests use (tests/test_shading.py checks on the CPU that they contain what the mutations need) ------------------------
SUNS = ((0.0, 0.5, 0.866), (0.8, 0.0524, -0.6), (-0.2, 0.95, 0.1))          # sky: the reference's default, 3 degrees above the horizon, high
SHADE_SUNS = (SUNS[0], (-0.8, 0.364, 0.6), SUNS[2])                           # water: 20 degrees for the low one (at 3 degrees a third of a rough sea's
                                                                              #   normals face away from the sun and a colour of exactly 0 has no relative bound)
TURBIDITIES = (2.0, 2.5, 6.0)
CAM = (3.0, 40.0, -5.0)
# Jerlov I as the reference ships it, and Jerlov III with the coastal scattering coefficient b(514 nm) = 0.219 (WaterSurfaceMesh.h:339-363)
WATERS = (None, dict(absorb=(0.520, 0.120, 0.135), b514=0.219))


def water_fields(kind):
    """Keyword fields for watersurfacerendering_amd.water_params of one of WATERS."""
    if kind is None:
        return {}
    b = [kind["b514"] * ((-0.00113 * nm + 1.62517) / (-0.00113 * 514.0 + 1.62517)) for nm in (680.0, 550.0, 440.0)]
    return dict(absorb=kind["absorb"], scatter=b, backscatter=[0.01829 * float(f32(x)) + 0.00006 for x in b])


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _around(axis, angles, phases):
    """Unit vectors at the given angles from `axis`, at the given phases around it."""
    axis = unit(axis)
    a = unit(np.cross(axis, (0.31, 0.2, 0.93)))
    b = np.cross(axis, a)
    angles, phases = np.asarray(angles)[:, None], np.asarray(phases)[:, None]
    return np.cos(angles) * axis + np.sin(angles) * (np.cos(phases) * a + np.sin(phases) * b)


EDGE = float(np.arccos(0.997))          # 4.44 degrees: where the sun disk's smoothstep starts


def sky_directions(sun, count=4099, seed=11):
    """Directions for ocean_sky_radiance: random over the sphere (not normalised: lengths 0.1 .. 10), the zenith, the horizon, below it, the
    sun itself, a ring across each smoothstep edge (0.997 and 1.0)."""
    rng = np.random.default_rng(seed)
    ph = np.linspace(0.0, 2 * np.pi, 64, endpoint=False)
    crafted = [np.array([[0, 1, 0], [0, 3, 0], [1, 0, 0], [0, 0, -2], [1, 0, 1], [0.3, -0.4, 0.5], [0, -1, 0], [1, 1e-4, 0], [1, -1e-4, 0.5]], dtype=np.float64),
               unit(sun)[None, :], 2.5 * unit(sun)[None, :],
               _around(sun, EDGE + np.linspace(-2e-3, 2e-3, 12), ph[::5][:12]), _around(sun, np.linspace(0.0, 3e-3, 12), ph[::5][:12]),
               _around(sun, np.linspace(0.0, EDGE, 8), ph[::8] + 1.0)]
    crafted = np.concatenate(crafted)
    rnd = unit(rng.normal(size=(count - len(crafted), 3))) * rng.uniform(0.1, 10.0, size=(count - len(crafted), 1))
    return np.concatenate([crafted, rnd]).astype(f32)


def shade_rows(sun, cam=CAM, count=4000, seed=5):
    """(pos, nrm, tags) for ocean_shade_points: `count` random vertices of a rough sea ahead of `cam` (x beyond it: the suns of SHADE_SUNS
    have their specular points beside or behind that patch, so that the glitter -- where the sun disk's slope of 333 makes the relative
    bound large -- comes from the crafted rows and stays under the cap on such points), then the crafted rows; tags names the index range
    of every crafted family."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(cam, dtype=np.float64)
    sun = unit(sun)
    pos = np.concatenate([cam[0] + rng.uniform(20, 620, (count, 1)), rng.normal(0, 1.5, (count, 1)), cam[2] + rng.uniform(-300, 300, (count, 1)),
                          rng.uniform(-0.2, 1.2, (count, 1))], axis=1)
    sl = rng.normal(0, 0.1, (count, 2))
    nrm = np.concatenate([-sl[:, :1], np.ones((count, 1)), -sl[:, 1:], np.zeros((count, 1))], axis=1)
    nrm[:, :3] = unit(nrm[:, :3]) * rng.uniform(0.5, 2.0, (count, 1))           # the call normalises
    P, N, tags = [pos], [nrm], {"random": (0, count)}

    def add(name, p, n, w=0.5):
        p, n = np.atleast_2d(np.asarray(p, dtype=np.float64)), np.atleast_2d(np.asarray(n, dtype=np.float64))
        p = np.concatenate([p, np.full((len(p), 1), w)], axis=1) if p.shape[1] == 3 else p
        n = np.concatenate([n, np.zeros((len(n), 1))], axis=1)
        start = sum(len(x) for x in P)
        P.append(p); N.append(n)
        tags[name] = (start, start + len(p))

    up = np.array([0.0, 1.0, 0.0])
    # straight down on a level surface: normal incidence (dot(n, V) = 1)
    add("above", [[cam[0], 0.0, cam[2]], [cam[0], -1.5, cam[2]]], [up, 2 * up])
    # grazing views of a level surface, 0.05 .. 8 degrees above the horizon: the reflection is as close to it (kBias)
    az = np.linspace(0.0, 2 * np.pi, 48, endpoint=False)
    dist = cam[1] / np.tan(np.radians(np.geomspace(0.05, 8.0, 48)))
    add("grazing", np.stack([cam[0] + dist * np.cos(az), np.zeros(48), cam[2] + dist * np.sin(az)], axis=1), np.tile(up, (48, 1)))
    # normals that face away from the camera but still towards the sun: dot(n, V) <= 0, the reference Fresnel's first branch
    p = np.stack([cam[0] + 200 * np.cos(az[::6]), np.zeros(8), cam[2] + 200 * np.sin(az[::6])], axis=1)
    view = unit(cam - p)
    away = unit(0.5 * up - unit(view * np.array([1.0, 0.0, 1.0])))
    assert ((away * view).sum(axis=1) < -0.05).all() and (away[:, 1] > 0.1).all()
    add("backfacing", p, away)
    # normals that mirror the camera into the sun (r = sun, Blinn-Phong at its peak), and rings across both smoothstep edges around them
    p = np.stack([cam[0] + 90 * np.cos(az[:8] * 6 + 0.1), rng.normal(0, 1, 8), cam[2] + 90 * np.sin(az[:8] * 6 + 0.1)], axis=1)
    view = unit(cam - p)
    mirror = unit(sun + view)
    ok = mirror[:, 1] > 0.2
    add("mirror", p[ok], mirror[ok])
    for name, ang in (("edge_outer", EDGE / 2 + np.linspace(-1e-3, 1e-3, 8)), ("edge_inner", np.linspace(0.0, 1.5e-3, 8))):
        ring = np.stack([_around(mirror[i], [ang[i]], [az[i] * 3])[0] for i in range(8)])
        add(name, p[ok], ring[ok])
    # foam: the Jacobian slot negative
    add("foam", [[20.0, 0.3, 30.0], [-45.0, -0.2, 12.0]], [unit([0.1, 1, -0.2]), unit([-0.3, 1, 0.1])], w=-0.25)
    return np.concatenate(P).astype(f32), np.concatenate(N).astype(f32), tags
