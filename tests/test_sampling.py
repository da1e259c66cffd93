"""Do the light, bounce and AO samplers have the distribution the estimator's derivation needs? The
bit-for-bit tests hold the host statements, the device kernels and the numpy models to one another,
and all three are written from one text; here mrth_shadow_rays, mrth_path_extend and mrth_ao_rays
(and the float32 numpy models of light_util / path_util) are held to something none of them was
written from: float64 restatements with a first-order bound per sample (tests/radiometry_util.py),
the moments, chi-squares, strata and correlations of the distributions themselves, and frames whose
expected value has a closed form. tests/test_gpu_sampling.py runs the same checks on the device.

Every `check_*` takes an implementation (Host or Model here, Device there), prints the figures it
asserts on (`-s` shows them; DESIGN section 19 records them) and is deterministic: the seeds are
fixed. A statistic must lie within 5 standard errors under independence; a chi-square below the
1 - 10^-6 quantile.
"""
import functools

import numpy as np
import pytest

import mrt
import mrt.host

import light_util as L
import path_util as P
import radiometry_util as R
import test_path as TP

F = np.float32
SLOTS = 65536
DEPTH = 3
LIGHT = (1.5, -2.0, 6.0)   # at least 2 away from every backed-off point: no ray is degenerate
MAX_DIST = 100.0
EDGE_MARGIN = 2.0 ** -20
GOLDEN = 0x9E3779B9


# ---------------------------------------------------------------- the implementations
class Host:
    name = "host"
    shadow = staticmethod(lambda rays, res, S, light, radius, seed: mrt.host.shadow_rays(rays, res, S, light, radius, seed=seed))
    extend = staticmethod(mrt.host.path_extend)
    ao = staticmethod(lambda rays, res, scene, S, max_dist, seed: mrt.host.ao_rays(rays, res, scene, max_dist, S, seed))
    frame_impl = mrt.host


class Model:
    name = "model"
    shadow = staticmethod(lambda rays, res, S, light, radius, seed: L.shadow_rays(rays, res, S, light, radius, seed)[0])
    extend = staticmethod(P.Model.path_extend)
    ao = None   # oracle/raygen_oracle.py restates the AO kernel in float64 already: no float32 model to hold
    frame_impl = P.Model


IMPLS = [Host, Model]


# ---------------------------------------------------------------- the tables
def _triangle(n, integer):
    """Two edges (u, v) with u x v parallel to n; from integer n all three are exact in float32, so
    that components of equal magnitude come out of the scene's cross product and normalisation equal."""
    n = np.asarray(n, np.float64)
    u = np.array([n[1], -n[0], 0.0]) if (n[0] or n[1]) else np.array([0.0, n[2], -n[1]])
    if not integer:
        u /= np.linalg.norm(u)
    return u, np.cross(n, u)


SPECIAL = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),   # +- each axis
           (2, 2, 1), (2, -2, 1), (-2, 2, -1),                                    # |nx| = |ny| largest
           (1, 2, 2), (1, -2, 2), (-1, 2, -2),                                    # |ny| = |nz| largest
           (1, 1, 1), (-1, 1, -1),                                                # all three equal
           (1, 1, 0), (0, 1, 1), (1, 0, 1), (0, 3, 4), (3, 0, -4)]                # one zero component


@functools.lru_cache(maxsize=None)
def table():
    """(scene, normals float32 [64, 3], material uint32 [64]): the scene's own triangle normals, so
    that mrth_ao_rays (which takes a scene) and mrt_path_extend (which takes a table) read the same."""
    rng = np.random.default_rng(19)
    rand = rng.normal(size=(64 - len(SPECIAL), 3))
    verts = []
    for k, n in enumerate(list(SPECIAL) + list(rand / np.linalg.norm(rand, axis=1, keepdims=True))):
        u, v = _triangle(n, k < len(SPECIAL))
        at = np.array([k % 8, k // 8, 0.0])
        verts += [at, at + u, at + v]
    scene = mrt.Scene.from_arrays(np.array(verts, F), np.arange(192, dtype=np.int32).reshape(-1, 3))
    normals = np.ascontiguousarray(scene.arrays()[2], F)
    normals.setflags(write=False)
    return scene, normals, scene.tri_colors()[0]


def test_the_normal_table_holds_the_edges():
    _, n, _ = table()
    a = np.abs(n)
    assert len(n) == 64 and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    for k, want in enumerate(SPECIAL):
        assert np.allclose(n[k], np.array(want) / np.linalg.norm(want), atol=1e-6), k
    assert all(a[k, 0] == a[k, 1] > a[k, 2] for k in (6, 7, 8))     # exact float32 ties: the order of the
    assert all(a[k, 1] == a[k, 2] > a[k, 0] for k in (9, 10, 11))   # perpendicular's tests decides
    assert all(a[k, 0] == a[k, 1] == a[k, 2] for k in (12, 13))
    assert all((a[k] == 0).sum() == 1 for k in range(14, 19)) and all((a[k] == 0).sum() == 2 for k in range(6))


@functools.lru_cache(maxsize=None)
def inputs(n, seed=5):
    """n traced rays (float32 [n, 8], int32 [n, 4]), read-only: triangle k % 64, met from the front by
    even rounds of the table and from behind by odd ones (|cos| >= 0.1, so float32 and float64 turn the
    normal alike), origins in [-1, 1]^3, t in [0.5, 2); every 17th a miss."""
    _, normals, _ = table()
    rng = np.random.default_rng(seed)
    ids = np.arange(n) % 64
    nrm = normals[ids].astype(np.float64)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = (d * nrm).sum(axis=1)
    want = np.where((np.arange(n) // 64) % 2 == 0, -1.0, 1.0) * np.maximum(np.abs(c), 0.1 + 0.8 * rng.random(n))
    tangent = d - c[:, None] * nrm
    tangent /= np.linalg.norm(tangent, axis=1, keepdims=True)
    d = want[:, None] * nrm + np.sqrt(1 - want * want)[:, None] * tangent
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    rays[:, 4:7] = d
    rays[:, 7] = MAX_DIST
    res = np.zeros((n, 4), np.int32)
    res[:, 0] = np.where(np.arange(n) % 17 == 16, -1, ids)
    res[:, 1] = rng.uniform(0.5, 2.0, n).astype(F).view(np.int32)
    rays.setflags(write=False)
    res.setflags(write=False)
    return rays, res


def wrapping_seed(vertex):
    """seed + vertex * 0x9e3779b9 + key passes 2^32 at key 16."""
    return (0xFFFFFFF0 - vertex * GOLDEN) & 0xFFFFFFFF


SEEDS = {"seed1-r0.5": (lambda vertex: 1, 0.5), "wrap-r1": (wrapping_seed, 1.0)}


def figures(label, **kw):
    print("FIG " + label + ": " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in kw.items()))


# ---------------------------------------------------------------- A. each sample against float64
def within_bound(got, v, e, use):
    """The worst |got - v| / e over the slots `use`; every entry with e == 0 must be equal."""
    diff = np.abs(np.asarray(got, np.float64) - v)[use]
    e = e[use]
    assert np.isfinite(e).all() and np.isfinite(diff).all()
    assert (diff[e == 0] == 0).all()
    ratio = float((diff[e > 0] / e[e > 0]).max())
    assert ratio <= 1.0, f"a sample is {ratio:.3g} of its bound away from the float64 restatement"
    return ratio


def unit_length(rays, use):
    worst = float(np.abs(np.linalg.norm(rays[use, 4:7].astype(np.float64), axis=1) - 1.0).max())
    assert worst <= 4 * R.EPS, worst
    return worst


# ---------------------------------------------------------------- B. the distributions
def moments(label, table_):
    out = {}
    for name, values, mean, var in table_:
        z = R.z_score(values, mean, var)
        out["z " + name] = z
        assert abs(z) <= 5.0, (label, name, z)
    return out


def cube_checks(label, pos):
    """pos float64 [n, 3], recovered from rays: moments, range (the caller allows the recovery's own
    error), and the 16 x 16 chi-squares of the three coordinate pairs."""
    out = moments(label, [(f"E[{c}]", pos[:, k], 0.0, 1 / 3) for k, c in enumerate("XYZ")] +
                  [(f"E[{c}^2]", pos[:, k] ** 2, 1 / 3, 4 / 45) for k, c in enumerate("XYZ")])
    cell = np.clip(((pos + 1.0) * 8.0).astype(np.int64), 0, 15)
    limit = R.chi2_quantile_1e6(255)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        chi = R.chi2_uniform(cell[:, a] * 16 + cell[:, b], 256)
        out[f"chi2 {'XYZ'[a]}{'XYZ'[b]}"] = chi
        assert chi <= limit, (label, a, b, chi)
    return out


def local_xyz(dirs, nf):
    perp, biperp, n = R.local_frame(nf)
    d = np.asarray(dirs, np.float64)
    return (d * perp).sum(axis=1), (d * biperp).sum(axis=1), (d * n).sum(axis=1)


def hemisphere_checks(label, x, y, z):
    out = moments(label, [("E[z]", z, 2 / 3, 1 / 18), ("E[z^2]", z * z, 1 / 2, 1 / 12), ("E[x]", x, 0.0, 1 / 4),
                                ("E[y]", y, 0.0, 1 / 4), ("E[x^2]", x * x, 1 / 4, 1 / 16)])
    u1, u2 = x * x + y * y, np.arctan2(y, x) / (2 * np.pi) % 1.0
    cell = np.clip((u1 * 16).astype(np.int64), 0, 15) * 16 + np.clip((u2 * 16).astype(np.int64), 0, 15)
    out["chi2 disk"] = R.chi2_uniform(cell, 256)
    assert out["chi2 disk"] <= R.chi2_quantile_1e6(255), (label, out["chi2 disk"])
    return out


def recovered_positions(rays, ref_e, light, radius):
    """(pos float64 [n, 3], its error bound [n]) of live shadow rays: (origin + direction * tmax - light) / radius."""
    r = np.asarray(rays, np.float64)
    pos = (r[:, 0:3] + r[:, 4:7] * r[:, 7:8] - np.asarray(light, F).astype(np.float64)) / float(F(radius))
    err = (ref_e[:, 0:3].sum(axis=1) + ref_e[:, 4:7].sum(axis=1) * np.abs(r[:, 7]) + ref_e[:, 7]) / float(F(radius))
    return pos, err


# ---------------------------------------------------------------- the light sampler: mrt_raygen_shadow
@functools.lru_cache(maxsize=None)
def light_reference(which, S, n):
    seed, radius = SEEDS[which]
    rays, res = inputs(n)
    return rays, res, seed(0), radius, R.shadow_rays(rays, res, S, LIGHT, radius, seed(0))


def check_light_sampler(impl, which):
    rays, res, seed, radius, ref = light_reference(which, 8, SLOTS // 8)
    got = np.asarray(impl.shadow(rays, res, 8, LIGHT, radius, seed), F).reshape(-1, 8)
    live = np.repeat(res[:, 0] != -1, 8)
    assert (got[~live, 7] == -1).all() and (got[:, 3] == 0).all()
    use = ~ref["edge"]
    ratio = within_bound(got, ref["v"], ref["e"], use)
    length = unit_length(got, use)
    pos, err = recovered_positions(got[live], ref["e"][live], LIGHT, radius)
    assert (np.abs(pos) <= 1.0 + err[:, None]).all()
    assert np.abs(pos - ref["pos"][live])[use[live]].max() <= 2 * err.max()
    out = cube_checks(which, pos)
    # the float64 reference alone passes the same conditions
    cube_checks(which + " (float64)", ref["pos"][live])
    assert (~use).mean() <= 1e-3
    figures(f"light sampler {impl.name} {which}", ratio=ratio, unit=length, edge_slots=int((~use).sum()), **out)
    return ratio


@pytest.mark.parametrize("which", list(SEEDS))
@pytest.mark.parametrize("impl", IMPLS, ids=lambda i: i.name)
def test_light_sampler_against_float64_and_its_distribution(impl, which):
    check_light_sampler(impl, which)


# ---------------------------------------------------------------- the vertex step: mrt_path_extend
@functools.lru_cache(maxsize=None)
def extend_reference(vertex, which, S=8):
    """Inputs of one extend call of SLOTS slots (or the most that S divides) and its float64 reference over the survivors."""
    seed, radius = SEEDS[which]
    _, normals, material = table()
    slots = SLOTS // S * S
    if vertex == 0:
        rays, res = inputs(slots // S)
        state, at = None, np.arange(slots) // S
    else:
        rays, res = inputs(slots, seed=5 + vertex)
        state = np.zeros((slots, 4), np.int32)
        state[:, :3] = np.ones((slots, 3), F).view(np.int32)
        state[:, 3] = np.arange(slots)
        at = np.arange(slots)
    tasks = np.flatnonzero(res[at, 0] >= 0)
    ref = R.path_extend(rays[at[tasks]], res[at[tasks]], tasks, normals, vertex, DEPTH, S, seed(vertex), LIGHT, radius, MAX_DIST)
    assert ref["clear"].all()
    call = dict(rays=rays, results=res, state=state, normals=normals, material=material, vertex=vertex, depth=DEPTH,
                num_samples=S, seed=seed(vertex), light_pos=LIGHT, light_radius=radius, light_color=(1.0, 0.5, 0.25),
                sky=(0.2, 0.4, 0.8), max_dist=MAX_DIST, compact=True)
    return call, tasks, radius, ref


_STEPS = {}


def step_of(impl, vertex, which, S=8):
    """The implementation's output of the case, computed once: (shadow [m, 8], bounce [m, 8] or None)."""
    key = (impl.name, vertex, which, S)
    if key not in _STEPS:
        call, tasks, _, _ = extend_reference(vertex, which, S)
        out = impl.extend(radiance=np.zeros((SLOTS, 4), F), **call)
        m = out["live"]
        assert m == len(tasks) and np.array_equal(out["state"][:m, 3], tasks)   # the survivors, in slot order
        _STEPS[key] = (np.array(out["shadow"][:m]), None if out["rays"] is None else np.array(out["rays"][:m]))
    return _STEPS[key]


def check_vertex_step(impl, vertex, which):
    call, tasks, radius, ref = extend_reference(vertex, which)
    shadow, bounce = step_of(impl, vertex, which)
    label = f"vertex {vertex} {which}"
    use = ~ref["edge_shadow"]
    fig = {"shadow ratio": within_bound(shadow, ref["shadow_v"], ref["shadow_e"], use), "shadow unit": unit_length(shadow, use),
           "shadow direction ratio": within_bound(shadow[:, 4:8], ref["shadow_v"][:, 4:8], ref["shadow_e"][:, 4:8], use)}
    pos, err = recovered_positions(shadow, ref["shadow_e"], LIGHT, radius)
    assert (np.abs(pos) <= 1.0 + err[:, None]).all()
    fig.update(cube_checks(label, pos))
    cube_checks(label + " (float64)", ref["pos"])
    edges = int((~use).sum())
    assert (bounce is None) == (vertex == DEPTH)
    if bounce is not None:
        use_b = ~ref["edge_bounce"]
        fig["bounce ratio"] = within_bound(bounce, ref["bounce_v"], ref["bounce_e"], use_b)
        fig["bounce direction ratio"] = within_bound(bounce[:, 4:7], ref["bounce_v"][:, 4:7], ref["bounce_e"][:, 4:7], use_b)
        fig["bounce unit"] = unit_length(bounce, use_b)
        x, y, z = local_xyz(bounce[:, 4:7], ref["nf"])
        assert (z >= 0).all()                       # no direction below its normal's horizon
        assert ((bounce[:, 4:7].astype(np.float64) * ref["nf"]).sum(axis=1) >= 0).all()
        fig.update(hemisphere_checks(label, x, y, z))
        hemisphere_checks(label + " (float64)", *local_xyz(ref["bounce_v"][:, 4:7], ref["nf"]))
        edges += int((~use_b).sum())
        # a path's light sample and its bounce do not move together
        for k, c in enumerate("XYZ"):
            for name, w in (("x", x), ("y", y)):
                rho = R.pearson(pos[:, k], w)
                fig[f"rho {c}{name}"] = rho * np.sqrt(len(w))
                assert abs(rho) <= 5.0 / np.sqrt(len(w)), (label, c, name, rho)
    assert edges <= 1e-3 * len(tasks)
    figures(f"{impl.name} {label}", edge_slots=edges, **fig)
    return fig


@pytest.mark.parametrize("which", list(SEEDS))
@pytest.mark.parametrize("vertex", [0, 1, DEPTH])
@pytest.mark.parametrize("impl", IMPLS, ids=lambda i: i.name)
def test_vertex_step_against_float64_and_its_distributions(impl, vertex, which):
    check_vertex_step(impl, vertex, which)


def correlations(label, a, b):
    """|rho| <= 5 / sqrt(n) between every component of the local (x, y) pairs a and b ([n, 2] each)."""
    out = {}
    for i, ni in enumerate("xy"):
        for j, nj in enumerate("xy"):
            rho = R.pearson(a[:, i], b[:, j])
            out[f"{ni}{nj}"] = rho * np.sqrt(len(a))
            assert abs(rho) <= 5.0 / np.sqrt(len(a)), (label, ni, nj, rho, len(a))
    return out


def check_independence(impl):
    """Bounces of one task at successive vertices, of neighbouring tasks at one vertex, and of
    neighbouring inputs' equal samples at vertex 0."""
    local = {}
    for vertex in (0, 1, 2):
        _, tasks, _, ref = extend_reference(vertex, "seed1-r0.5")
        x, y, _ = local_xyz(step_of(impl, vertex, "seed1-r0.5")[1][:, 4:7], ref["nf"])
        xy = np.full((SLOTS, 2), np.nan)
        xy[tasks] = np.stack([x, y], 1)
        local[vertex] = xy
    fig = {}
    for b in (0, 1):
        both = ~np.isnan(local[b][:, 0]) & ~np.isnan(local[b + 1][:, 0])
        fig.update({f"v{b}v{b + 1} {k}": v for k, v in correlations(f"vertex {b} and {b + 1}", local[b][both], local[b + 1][both]).items()})
    a, b = local[1][:-1], local[1][1:]
    both = ~np.isnan(a[:, 0]) & ~np.isnan(b[:, 0])
    fig.update({f"tasks {k}": v for k, v in correlations("tasks k and k + 1", a[both], b[both]).items()})
    a, b = local[0][:-8], local[0][8:]
    both = ~np.isnan(a[:, 0]) & ~np.isnan(b[:, 0])
    fig.update({f"inputs {k}": v for k, v in correlations("inputs k and k + 1", a[both], b[both]).items()})
    figures(f"independence {impl.name} (rho sqrt(n))", **fig)


@pytest.mark.parametrize("impl", IMPLS, ids=lambda i: i.name)
def test_bounces_are_independent_across_vertices_tasks_and_inputs(impl):
    check_independence(impl)


# ---------------------------------------------------------------- strata
def base_digits(n, base):
    k = 0
    while n:
        n //= base
        k += 1
    return k


def check_strata(impl, S, a, b):
    """At vertex 0 a pixel's S paths share one shift. With the shift (known from the float64 words)
    taken off, the S disk points (u1, u2) are the Halton points of indices 1..S: one per cell of the
    2^a x 3^b grid, S = 2^a 3^b, and the cube's third coordinates one per interval of width 2 / S. The
    Halton points are themselves lattice points k / 2^m, l / 3^n (m, n the digits of S) and so lie ON
    cell edges; half a lattice step is added to each coordinate first, which puts a correct point at
    the centre of a lattice cell, at least that half step from any edge of the coarser grid, and
    leaves a wrong one wherever it fell. A point within 2^-20 plus its own recovery error of a cell
    edge is left out with its pixel; the left-out share is capped at 0.1 %."""
    assert 2 ** a * 3 ** b == S
    call, tasks, radius, ref = extend_reference(0, "seed1-r0.5", S)
    shadow, bounce = step_of(impl, 0, "seed1-r0.5", S)
    x, y, _ = local_xyz(bounce[:, 4:7], ref["nf"])
    e_loc = ref["bounce_e"][:, 4:7].sum(axis=1)
    u1, u2 = x * x + y * y, np.arctan2(y, x) / (2 * np.pi)
    e1 = 2 * (np.abs(x) + np.abs(y)) * e_loc
    e2 = (np.abs(x) + np.abs(y)) * e_loc / np.maximum(u1, 1e-300) / (2 * np.pi)
    g1 = ((u1 - ref["shift"][:, 0] + 0.5 ** (base_digits(S, 2) + 1)) % 1.0) * 2 ** a
    g2 = ((u2 - ref["shift"][:, 1] + 0.5 * 3.0 ** -base_digits(S, 3)) % 1.0) * 3 ** b
    pos, perr = recovered_positions(shadow, ref["shadow_e"], LIGHT, radius)
    g3 = (((pos[:, 2] + 1.0) / 2.0 - ref["offset"][:, 2]) % 1.0) * S
    near = np.zeros(len(tasks), bool)
    for g, e, cells in ((g1, e1, 2 ** a), (g2, e2, 3 ** b), (g3, perr / 2, S)):
        near |= np.abs(g - np.round(g)) <= (EDGE_MARGIN + e) * cells
    pixels = len(tasks) // S
    assert len(tasks) == pixels * S and (tasks.reshape(pixels, S) // S == tasks[::S, None] // S).all()
    keep = ~near.reshape(pixels, S).any(axis=1)
    left_out = float(near.mean())
    assert left_out <= 1e-3, left_out
    disk = (np.floor(g1).astype(np.int64) * 3 ** b + np.floor(g2).astype(np.int64)).reshape(pixels, S)[keep]
    third = np.floor(g3).astype(np.int64).reshape(pixels, S)[keep]
    want = np.arange(S)[None, :]
    assert (np.sort(disk, axis=1) == want).all(), "a pixel's disk points do not fall one per cell"
    assert (np.sort(third, axis=1) == want).all(), "a pixel's third cube coordinates do not fall one per interval"
    # the float64 reference alone: no point near an edge at all
    r1 = ((ref["u"][:, 0] - ref["shift"][:, 0] + 0.5 ** (base_digits(S, 2) + 1)) % 1.0) * 2 ** a
    assert (np.abs(r1 - np.round(r1)) > EDGE_MARGIN * 2 ** a).all()
    figures(f"strata {impl.name} S={S}", pixels=int(keep.sum()), left_out=left_out)


@pytest.mark.parametrize("S,a,b", [(6, 1, 1), (36, 2, 2)])
@pytest.mark.parametrize("impl", IMPLS, ids=lambda i: i.name)
def test_a_pixels_paths_fall_one_per_cell(impl, S, a, b):
    check_strata(impl, S, a, b)


def occupancy(u, m):
    """Counts of S = 2^m points u [pixels, S, 2] (a quarter lattice step already added) in the elementary
    intervals 2^-j x 2^-(m - j), j = 0..m: int [pixels, m + 1, S]."""
    out = np.zeros((u.shape[0], m + 1, 2 ** m), np.int64)
    for j in range(m + 1):
        cell = np.floor(u[:, :, 0] * 2 ** j).astype(np.int64) * 2 ** (m - j) + np.floor(u[:, :, 1] * 2 ** (m - j)).astype(np.int64)
        for p in range(2 ** m):
            out[:, j, p] = (cell == p).sum(axis=1)
    return out


def check_sobol_pair(impl):
    """The cube's first two coordinates with the offset taken off are the reference's sobol2D with its
    `v2 << 1`. Whether that is a (0, m, 2)-net is not assumed: the occupancy of every elementary
    interval must be what the float64 restatement's is. Its points are multiples of 2^-m, so 2^-(m+2)
    is added: a correct point then sits a quarter step inside its cell."""
    found = {}
    for m in (2, 3, 4, 5, 6):
        S, n = 2 ** m, 256
        rays, res, seed, radius, ref = light_reference("seed1-r0.5", S, n)
        got = np.asarray(impl.shadow(rays, res, S, LIGHT, radius, seed), F).reshape(-1, 8)
        live = np.repeat(res[:, 0] != -1, S)
        pos, err = recovered_positions(got[live], ref["e"][live], LIGHT, radius)
        off = np.repeat(R.unit(R.hash_words(np.arange(n, dtype=np.uint64) + np.uint64(seed))[0]).v, S, axis=0)[live]
        nudge = 2.0 ** -(m + 2)
        u = ((pos[:, :2] + 1.0) / 2.0 - off[:, :2] + nudge) % 1.0
        assert err.max() / 2 + EDGE_MARGIN < nudge / 2    # no point can be near an edge of any interval
        want = occupancy(((R.sobol2d(S) + nudge) % 1.0)[None], m)
        have = occupancy(u.reshape(-1, S, 2), m)
        assert (have == want).all(), f"S = {S}: the elementary intervals are not occupied as the float64 restatement's"
        found[S] = [sorted(set(want[0, j].tolist())) for j in range(m + 1)]
    print("FIG sobol occupancy " + impl.name + ": " + "; ".join(f"S={S} counts per j {v}" for S, v in found.items()))
    return found


@pytest.mark.parametrize("impl", IMPLS, ids=lambda i: i.name)
def test_sobol_pair_occupies_the_elementary_intervals_as_the_restatement(impl):
    found = check_sobol_pair(impl)
    # what the occupancy is: one point in every elementary interval of every shape, so the
    # first 2^m points of the `<< 1` variant are a (0, m, 2)-net for m = 2..6
    for S, per_j in found.items():
        assert all(counts == [1] for counts in per_j), (S, per_j)


# ---------------------------------------------------------------- the AO generator
@functools.lru_cache(maxsize=None)
def ao_reference(S, n, seed):
    _, normals, _ = table()
    rays, res = inputs(n)
    return rays, res, R.ao_rays(rays, res, normals, S, 5.0, seed)


def check_ao(impl, seed):
    scene, _, _ = table()
    rays, res, ref = ao_reference(8, SLOTS // 8, seed)
    got = np.asarray(impl.ao(rays, res, scene, 8, 5.0, seed), F).reshape(-1, 8)
    use = ref["clear"]
    assert use.all()
    ratio = within_bound(got, ref["v"], ref["e"], use)
    directions = within_bound(got[:, 4:7], ref["v"][:, 4:7], ref["e"][:, 4:7], use)   # where cosf / sinf enter
    length = unit_length(got, use)
    assert ((got[:, 4:7].astype(np.float64) * ref["nf"]).sum(axis=1) >= 0).all()
    figures(f"ao {impl.name} seed {seed:#x}", ratio=ratio, direction_ratio=directions, unit=length)
    return ratio


def check_ao_hash_angle(impl):
    """One sample per input over 65 536 tasks: the direction's angle in the (perp, biperp) frame is the
    hash angle plus the first Halton point's 2 pi / 3; 64 bins."""
    scene, _, _ = table()
    rays, res, ref = ao_reference(1, SLOTS, 1)
    got = np.asarray(impl.ao(rays, res, scene, 1, 5.0, 1), F).reshape(-1, 8)
    x, y, _ = local_xyz(got[:, 4:7], ref["nf"])
    turn = (np.arctan2(y, x) / (2 * np.pi) - 1.0 / 3.0) % 1.0
    away = np.abs((turn - ref["angle"] + 0.5) % 1.0 - 0.5)
    assert away.max() <= 1e-5, away.max()
    chi = R.chi2_uniform(np.clip((turn * 64).astype(np.int64), 0, 63), 64)
    assert chi <= R.chi2_quantile_1e6(63), chi
    assert R.chi2_uniform(np.clip((ref["angle"] * 64).astype(np.int64), 0, 63), 64) <= R.chi2_quantile_1e6(63)
    figures(f"ao hash angle {impl.name}", chi2=chi, worst_turn_error=float(away.max()))


@pytest.mark.parametrize("seed", [1, 0xFFFFFFF0])
def test_ao_rays_against_float64(seed):
    check_ao(Host, seed)


def test_ao_hash_angle_is_uniform():
    check_ao_hash_angle(Host)


# ---------------------------------------------------------------- the closed forms, checked on their own
FLOOR = (-4.0, 4.0, -3.0, 5.0)
OCCLUDER = (-1.0, 1.0, -1.0, 1.0)


def test_chi_square_quantiles_against_wilson_and_hilferty():
    for k in R.CHI2_1E6:
        assert 0.0 < R.wilson_hilferty_1e6(k) - R.chi2_quantile_1e6(k) < 0.5


def test_form_factor_against_brute_force():
    assert abs(float(R.form_factor(0.0, 0.0, 1.0, *OCCLUDER)) - 0.55413) < 5e-6   # 4 / (pi sqrt 2) atan(1 / sqrt 2) = 0.5541264
    for px, py, c, want in ((0.0, 0.0, 1.0, None), (0.5, 0.0, 1.0, 0.49790), (2.0, 0.0, 1.0, 0.06983), (0.3, -0.45, 0.9999, None),
                            (-1.0, 1.0, 1.0, None), (0.2, 0.1, 1.0, None)):
        f = float(R.form_factor(px, py, c, *OCCLUDER))
        assert abs(f - R.form_factor_quadrature(px, py, c, *OCCLUDER)) < 1e-9, (px, py)
        assert want is None or abs(f - want) < 5e-6
    assert abs(float(R.form_factor(0.2, 0.1, 1.0, *FLOOR)) - R.form_factor_quadrature(0.2, 0.1, 1.0, *FLOOR)) < 1e-9


def test_visible_share_against_a_grid():
    """The clipped polygon's area against the defining condition counted over a 2000 x 2000 grid of the square."""
    px = np.array([-0.66, -0.3, 0.0, 0.25, 0.66, -1.2, 1.2])
    got = R.visible_share(px, 1e-4, 0.0, 1.0, 0.0, 2.0, 0.5)
    g = (np.arange(2000) + 0.5) / 2000 - 0.5
    X, Z = np.meshgrid(g, 2.0 + g, indexing="ij")
    for x, v in zip(px, got):
        crossing = x + (X - x) * (1.0 - 1e-4) / (Z - 1e-4)
        assert abs(v - (crossing > 0).mean()) < 1e-3, (x, v)
    assert got[-2] == 0.0 and got[-1] == 1.0 and abs(got[2] - 0.5) < 1e-4


def test_two_bounce_quadrature_has_converged():
    px, py = np.array([0.0, 0.6, -0.66, 0.3]), np.array([0.0, 0.0, 0.49, -0.2])
    a = R.two_bounce_term(px, py, np.full(4, 1e-4), OCCLUDER, 1.0, FLOOR, 16)
    b = R.two_bounce_term(px, py, np.full(4, 1e-4), OCCLUDER, 1.0, FLOOR, 32)
    assert np.abs(a - b).max() <= 1e-6 and (a > 0.01).all()


# ---------------------------------------------------------------- C. frames with a closed-form expectation
W, H, SAMPLES = 96, 72, 8
SKY, ALBEDO = np.array([0.2, 0.4, 0.8]), TP.ALBEDO
CAMERA = ((0.0, 0.0, 0.5), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 90.0, 0.01, 100.0)
FRAMES = {
    "sky": dict(tris=TP.rect(0.0, *FLOOR) + TP.fan(1.0, 1.0, (0.3, 0.4)), depth=1,
                scalars=dict(light_pos=(0.0, 0.0, 2.0), light_radius=0.5, light_color=(0.0, 0.0, 0.0), sky=tuple(SKY), max_dist=100.0)),
    "penumbra": dict(tris=TP.rect(0.0, *FLOOR) + TP.rect(1.0, -6.0, 0.0, -6.0, 6.0), depth=0,
                     scalars=dict(light_pos=(0.0, 0.0, 2.0), light_radius=0.5, light_color=(1.0, 1.0, 1.0), sky=(0.0, 0.0, 0.0), max_dist=100.0)),
    "two bounces": dict(tris=TP.rect(0.0, *FLOOR) + TP.fan(1.0, 1.0, (0.3, 0.4)), depth=2,
                        scalars=dict(light_pos=(0.0, 0.0, 2.0), light_radius=0.5, light_color=(0.0, 0.0, 0.0), sky=tuple(SKY), max_dist=100.0)),
}


def cpu_frame(impl, name):
    """(primary rays, results, slot_to_id, pixels, image [pixels, 4], shadow-frame pixels or None): the
    frame with every trace done by the oracle, one batch seeded like a Renderer's first."""
    f = FRAMES[name]
    scene, bufs, normals, material = TP.world_of(f["tris"])
    assert (material == 0xFFBFBFBF).all()
    prim, s2i = mrt.primary_rays(mrt.host.Camera(*CAMERA), W, H)
    trace = TP.oracle_trace(bufs)
    pres = trace(prim, False)
    radiance, _ = P.render_batch(impl.frame_impl, trace, prim, pres, 0, W * H, normals, material, SAMPLES, f["depth"],
                                 mrt.AO_SEED, True, f["scalars"])
    px, image = impl.frame_impl.path_resolve(SAMPLES, s2i, pres, radiance, W * H, want_image=True)
    lit = None
    if name == "penumbra":
        rays = mrt.host.shadow_rays(prim, pres, SAMPLES, f["scalars"]["light_pos"], f["scalars"]["light_radius"], seed=mrt.AO_SEED)
        lit = mrt.host.reconstruct_lit(SAMPLES, s2i, prim, pres, trace(rays, True), normals, material,
                                       f["scalars"]["light_pos"], W * H)
    return prim, pres, s2i, px, image, lit


def expectation(name, p):
    """(mu [n, 3], M [n, 3]) at the backed-off floor points p float64 [n, 3]: the expected pixel and
    the largest value one path can have."""
    c = 1.0 - p[:, 2]
    if name == "penumbra":
        to_light = np.array([0.0, 0.0, 2.0]) - p
        k = to_light[:, 2] / np.linalg.norm(to_light, axis=1)        # nf = (0, 0, 1)
        v = R.visible_share(p[:, 0], p[:, 2], 0.0, 1.0, 0.0, 2.0, 0.5)
        top = (ALBEDO * k)[:, None] * np.ones(3)
        return top * v[:, None], top
    escape = 1.0 - R.form_factor(p[:, 0], p[:, 1], c, *OCCLUDER)
    mu = ALBEDO * escape
    if name == "two bounces":
        mu = mu + ALBEDO * ALBEDO * R.two_bounce_term(p[:, 0], p[:, 1], p[:, 2], OCCLUDER, 1.0, FLOOR, 24)
    return mu[:, None] * SKY[None, :], np.tile(ALBEDO * SKY, (len(p), 1))


def check_frame(name, prim, pres, s2i, px, image, lit, who):
    """z = sum(g - mu) / sqrt(sum v) per channel, v = (M - mu) mu / S the Bhatia-Davis bound of a path's
    value in [0, M]: stratification only lowers the true variance."""
    hit = pres[:, 0] != -1
    t = pres[:, 1].view(F).astype(np.float64)
    p = prim[:, 0:3].astype(np.float64) + prim[:, 4:7].astype(np.float64) * (t - 1e-4)[:, None]
    use = hit & (pres[:, 0] < 2)                                    # on the floor
    if name == "penumbra":
        use &= np.abs(p[:, 0]) > 2 * (1.0 / H)                      # two pixels (1 / 72 wide on the floor) off the projected edge
    left_out = 1.0 - use.mean()
    assert left_out <= 0.05, left_out
    mu, top = expectation(name, p[use])
    g = image[s2i[use], :3].astype(np.float64)
    assert (image[s2i[hit], 3] == 1.0).all() and (g >= 0).all() and (g <= top * (1 + 1e-6)).all()
    var = (top - mu) * mu / SAMPLES
    fig = {"left_out": float(left_out)}
    for c, ch in enumerate("rgb"):
        if top[:, c].max() == 0:
            continue
        z = (g[:, c] - mu[:, c]).sum() / np.sqrt(var[:, c].sum())
        fig[f"z {ch}"] = float(z)
        fig[f"5se/mean {ch}"] = float(5 * np.sqrt(var[:, c].sum()) / mu[:, c].sum())
        assert abs(z) <= 5.0, (name, ch, z)
    if lit is not None:   # the same frame as a RAY_SHADOW frame: one byte step
        assert np.abs(TP.channels(px) - TP.channels(lit)).max() <= 1
    figures(f"frame {who} {name}", **fig)
    return fig


@pytest.mark.parametrize("name", list(FRAMES))
@pytest.mark.parametrize("impl", IMPLS, ids=lambda i: i.name)
def test_frame_mean_against_its_closed_form(impl, name):
    check_frame(name, *cpu_frame(impl, name), impl.name)
