"""What the six entry points of the two ICP refinements refuse, and with which words: (entry, case, code, text), recorded on an
MI355X from the revision before the two refinements shared one driver.  code: the return value; text: the
whole of plade_last_error after the call.  case: what is wrong with an otherwise valid call on the small scenes below --
  null     the argument handed over as NULL ("tgt", "src", "T", "out"; the seams: "center", "moments")
  n_t n_s  the count handed over instead of the cloud's
  stride   the source stride of plade_icp_linearize
  nan      which of "T", "center", "tgt", "src" get a NaN (T[0][3], center[1], row 7's y)
  scene    "one_point": a target of one point fifty times; "far": the source moved 1000 units away; "line": both clouds on the
           x axis, normals (0, 0, 1)
  prm      fields of the params struct ("nan" / "inf" for the reals that a literal cannot hold)
  dist epsilon   the seams' arguments
A row with two faults pins the order of the checks.  tests/test_gpu_refine_messages.py replays the rows."""
import ctypes as C

import numpy as np

import plade_amd

ENTRIES = ("refine_icp", "refine_icp_dev", "icp_linearize", "refine_gicp", "refine_gicp_dev", "gicp_linearize")


def corner(n, seed):
    """n points x y z nx ny nz on the three faces of the unit cube that meet at the origin (a third each, seeded)"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 6), np.float32)
    face = np.arange(n) % 3
    uv = rng.uniform(0.0, 1.0, size=(n, 2)).astype(np.float32)
    for f in range(3):
        m = face == f
        a[m, (f + 1) % 3] = uv[m, 0]
        a[m, (f + 2) % 3] = uv[m, 1]
        a[m, 3 + f] = 1.0
    return a


def line(n, seed):
    a = np.zeros((n, 6), np.float32)
    a[:, 0] = np.random.default_rng(seed).uniform(-2, 2, size=n)
    a[:, 5] = 1
    return a


def scene(name):
    """(target, source) of a case: a few hundred points each"""
    if name == "line":
        return line(300, 0), line(300, 0)
    tgt, src = corner(600, 1), corner(300, 2)
    if name == "one_point":
        tgt = np.ascontiguousarray(np.repeat(tgt[:1], 50, axis=0))
    if name == "far":
        src[:, :3] += 1000.0
    return tgt, src


# the parameters of the refinement that ends the replay (the corner is too sparse for the automatic distances)
GOOD = {"max_dist": 0.2, "min_dist": 0.05, "min_correspondences": 10}


def _params(gicp, fields):
    prm = (plade_amd.GicpParams if gicp else plade_amd.IcpParams)()
    L = plade_amd.load_library()
    (L.plade_gicp_default_params if gicp else L.plade_icp_default_params)(C.byref(prm))
    for k, v in fields.items():
        setattr(prm, k, float(v) if isinstance(v, str) else v)
    return prm


def call(ctx, entry, case):
    """The call of `case` on the entry point `entry` through the C ABI: (return code, plade_last_error, T_out or None)."""
    L, h = ctx.L, ctx.h
    gicp, seam, dev = "gicp" in entry, entry.endswith("linearize"), entry.endswith("_dev")
    tgt, src = scene(case.get("scene", "corner"))
    if entry == "icp_linearize":
        src = np.ascontiguousarray(src[:, :3])
    nan = case.get("nan", ())
    if "tgt" in nan:
        tgt[7, 1] = np.nan
    if "src" in nan:
        src[7, 1] = np.nan
    T = np.eye(4, dtype=np.float64 if seam else np.float32)
    if "T" in nan:
        T[0, 3] = np.nan
    center = np.zeros(3, np.float64)
    if "center" in nan:
        center[1] = np.nan
    n_t, n_s = case.get("n_t", len(tgt)), case.get("n_s", len(src))
    null = case.get("null")
    p = lambda name, a: None if null == name else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    out = None
    if seam:
        mom = np.zeros(30 if gicp else 29, np.float64)
        corr = np.empty(len(src), np.int32)
        dist = float(case.get("dist", 0.1))
        if gicp:
            rc = L.plade_gicp_linearize(h, p("tgt", tgt), n_t, p("src", src), n_s, p("T", T), p("center", center), dist,
                                        float(case.get("epsilon", 0.0)), p("corr", corr), p("moments", mom))
        else:
            rc = L.plade_icp_linearize(h, p("tgt", tgt), n_t, p("src", src), n_s, case.get("stride", 3), p("T", T), p("center", center),
                                       dist, p("corr", corr), p("moments", mom))
    else:
        prm = _params(gicp, case.get("prm", {}))
        res = (plade_amd.GicpResult if gicp else plade_amd.IcpResult)()
        out = np.zeros((4, 4), np.float32)
        if dev:
            ct, cs = ctx.upload(tgt), ctx.upload(src)
            fn = L.plade_refine_gicp_dev if gicp else L.plade_refine_icp_dev
            rc = fn(h, None if null == "tgt" else ct.h, None if null == "src" else cs.h, p("T", T), C.byref(prm), p("out", out), C.byref(res))
            ct.free(); cs.free()
        else:
            fn = L.plade_refine_gicp if gicp else L.plade_refine_icp
            rc = fn(h, p("tgt", tgt), n_t, p("src", src), n_s, p("T", T), C.byref(prm), p("out", out), C.byref(res))
    return rc, L.plade_last_error(h).decode(errors="replace"), out


CASES = [
    ('refine_icp', {'null': 'tgt'}, -1, 'plade_refine_icp: bad argument'),
    ('refine_icp', {'null': 'src'}, -1, 'plade_refine_icp: bad argument'),
    ('refine_icp', {'null': 'T'}, -1, 'plade_refine_icp: bad argument'),
    ('refine_icp', {'null': 'out'}, -1, 'plade_refine_icp: bad argument'),
    ('refine_icp', {'n_t': 0}, -1, 'plade_refine_icp: empty cloud'),
    ('refine_icp', {'n_s': 0}, -1, 'plade_refine_icp: empty cloud'),
    ('refine_icp', {'nan': ('T',)}, -1, 'refine_icp: T_in must be finite'),
    ('refine_icp', {'nan': ('tgt',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('refine_icp', {'nan': ('src',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('refine_icp', {'scene': 'one_point'}, -1, "refine_icp: the target's bounding box is a single point"),
    ('refine_icp', {'prm': {'source_leaf': -1.0}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp', {'prm': {'source_leaf': 'inf'}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp', {'prm': {'max_dist': -1.0}}, -1, 'refine_icp: max_dist must be finite and >= 0'),
    ('refine_icp', {'prm': {'max_dist': 'inf'}}, -1, 'refine_icp: max_dist must be finite and >= 0'),
    ('refine_icp', {'prm': {'min_dist': -1.0}}, -1, 'refine_icp: min_dist must be finite and >= 0'),
    ('refine_icp', {'prm': {'min_dist': 'inf'}}, -1, 'refine_icp: min_dist must be finite and >= 0'),
    ('refine_icp', {'prm': {'eps_rotation': -1.0}}, -1, 'refine_icp: eps_rotation must be finite and >= 0'),
    ('refine_icp', {'prm': {'eps_rotation': 'inf'}}, -1, 'refine_icp: eps_rotation must be finite and >= 0'),
    ('refine_icp', {'prm': {'eps_translation': -1.0}}, -1, 'refine_icp: eps_translation must be finite and >= 0'),
    ('refine_icp', {'prm': {'eps_translation': 'inf'}}, -1, 'refine_icp: eps_translation must be finite and >= 0'),
    ('refine_icp', {'prm': {'source_leaf': 'nan'}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp', {'prm': {'max_iterations': -1}}, -1, 'refine_icp: max_iterations and min_correspondences must be >= 0'),
    ('refine_icp', {'prm': {'min_correspondences': -1}}, -1, 'refine_icp: max_iterations and min_correspondences must be >= 0'),
    ('refine_icp', {'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, 'refine_icp: min_dist > max_dist'),
    ('refine_icp', {'prm': {'max_dist': 1.0, 'min_dist': 1e-06}}, -1, 'refine_icp: more than 16 stages (max_dist / min_dist > 2^15)'),
    ('refine_icp', {'prm': {'source_leaf': 1e-07}}, -5, 'voxel: more than 2^18 leaves along one axis (PCL would refuse this leaf size too)'),
    ('refine_icp', {'null': 'tgt', 'n_s': 0}, -1, 'plade_refine_icp: bad argument'),
    ('refine_icp', {'n_t': 0, 'nan': ('T',)}, -1, 'plade_refine_icp: empty cloud'),
    ('refine_icp', {'nan': ('T', 'tgt')}, -1, 'refine_icp: T_in must be finite'),
    ('refine_icp', {'nan': ('tgt',), 'prm': {'max_dist': -1.0}}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('refine_icp', {'nan': ('T',), 'prm': {'max_dist': -1.0}}, -1, 'refine_icp: T_in must be finite'),
    ('refine_icp', {'prm': {'source_leaf': -1.0, 'max_dist': -1.0}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp', {'prm': {'eps_translation': -1.0, 'max_iterations': -1}}, -1, 'refine_icp: eps_translation must be finite and >= 0'),
    ('refine_icp', {'prm': {'max_iterations': -1}, 'scene': 'one_point'}, -1, 'refine_icp: max_iterations and min_correspondences must be >= 0'),
    ('refine_icp', {'scene': 'one_point', 'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, "refine_icp: the target's bounding box is a single point"),
    ('refine_icp', {'scene': 'far'}, -4, 'refine_icp: too few correspondences'),
    ('refine_icp', {'scene': 'line', 'prm': {'min_correspondences': 10}}, -4, 'refine_icp: degenerate geometry (the system is singular)'),
    ('refine_icp_dev', {'null': 'tgt'}, -1, 'plade_refine_icp_dev: bad argument'),
    ('refine_icp_dev', {'null': 'src'}, -1, 'plade_refine_icp_dev: bad argument'),
    ('refine_icp_dev', {'null': 'T'}, -1, 'plade_refine_icp_dev: bad argument'),
    ('refine_icp_dev', {'null': 'out'}, -1, 'plade_refine_icp_dev: bad argument'),
    ('refine_icp_dev', {'nan': ('T',)}, -1, 'refine_icp: T_in must be finite'),
    ('refine_icp_dev', {'scene': 'one_point'}, -1, "refine_icp: the target's bounding box is a single point"),
    ('refine_icp_dev', {'prm': {'source_leaf': -1.0}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'source_leaf': 'inf'}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'max_dist': -1.0}}, -1, 'refine_icp: max_dist must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'max_dist': 'inf'}}, -1, 'refine_icp: max_dist must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'min_dist': -1.0}}, -1, 'refine_icp: min_dist must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'min_dist': 'inf'}}, -1, 'refine_icp: min_dist must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'eps_rotation': -1.0}}, -1, 'refine_icp: eps_rotation must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'eps_rotation': 'inf'}}, -1, 'refine_icp: eps_rotation must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'eps_translation': -1.0}}, -1, 'refine_icp: eps_translation must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'eps_translation': 'inf'}}, -1, 'refine_icp: eps_translation must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'source_leaf': 'nan'}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'max_iterations': -1}}, -1, 'refine_icp: max_iterations and min_correspondences must be >= 0'),
    ('refine_icp_dev', {'prm': {'min_correspondences': -1}}, -1, 'refine_icp: max_iterations and min_correspondences must be >= 0'),
    ('refine_icp_dev', {'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, 'refine_icp: min_dist > max_dist'),
    ('refine_icp_dev', {'prm': {'max_dist': 1.0, 'min_dist': 1e-06}}, -1, 'refine_icp: more than 16 stages (max_dist / min_dist > 2^15)'),
    ('refine_icp_dev', {'prm': {'source_leaf': 1e-07}}, -5, 'voxel: more than 2^18 leaves along one axis (PCL would refuse this leaf size too)'),
    ('refine_icp_dev', {'null': 'src', 'nan': ('T',)}, -1, 'plade_refine_icp_dev: bad argument'),
    ('refine_icp_dev', {'nan': ('T',), 'prm': {'max_dist': -1.0}}, -1, 'refine_icp: T_in must be finite'),
    ('refine_icp_dev', {'prm': {'source_leaf': -1.0, 'max_dist': -1.0}}, -1, 'refine_icp: source_leaf must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'eps_translation': -1.0, 'max_iterations': -1}}, -1, 'refine_icp: eps_translation must be finite and >= 0'),
    ('refine_icp_dev', {'prm': {'max_iterations': -1}, 'scene': 'one_point'}, -1, 'refine_icp: max_iterations and min_correspondences must be >= 0'),
    ('refine_icp_dev', {'scene': 'one_point', 'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, "refine_icp: the target's bounding box is a single point"),
    ('refine_icp_dev', {'scene': 'far'}, -4, 'refine_icp: too few correspondences'),
    ('refine_icp_dev', {'scene': 'line', 'prm': {'min_correspondences': 10}}, -4, 'refine_icp: degenerate geometry (the system is singular)'),
    ('icp_linearize', {'null': 'tgt'}, -1, 'plade_icp_linearize: bad argument'),
    ('icp_linearize', {'null': 'src'}, -1, 'plade_icp_linearize: bad argument'),
    ('icp_linearize', {'null': 'T'}, -1, 'plade_icp_linearize: bad argument'),
    ('icp_linearize', {'null': 'center'}, -1, 'plade_icp_linearize: bad argument'),
    ('icp_linearize', {'null': 'moments'}, -1, 'plade_icp_linearize: bad argument'),
    ('icp_linearize', {'n_t': 0}, -1, 'plade_icp_linearize: empty cloud or stride < 3'),
    ('icp_linearize', {'n_s': 0}, -1, 'plade_icp_linearize: empty cloud or stride < 3'),
    ('icp_linearize', {'stride': 2}, -1, 'plade_icp_linearize: empty cloud or stride < 3'),
    ('icp_linearize', {'nan': ('T',)}, -1, 'plade_icp_linearize: T must be finite'),
    ('icp_linearize', {'nan': ('center',)}, -1, 'plade_icp_linearize: center must be finite'),
    ('icp_linearize', {'nan': ('tgt',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('icp_linearize', {'nan': ('src',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('icp_linearize', {'dist': 0.0}, -1, 'plade_icp_linearize: dist must be finite and > 0'),
    ('icp_linearize', {'dist': 'inf'}, -1, 'plade_icp_linearize: dist must be finite and > 0'),
    ('icp_linearize', {'null': 'center', 'n_t': 0}, -1, 'plade_icp_linearize: bad argument'),
    ('icp_linearize', {'n_s': 0, 'dist': 0.0}, -1, 'plade_icp_linearize: empty cloud or stride < 3'),
    ('icp_linearize', {'dist': 0.0, 'nan': ('T',)}, -1, 'plade_icp_linearize: dist must be finite and > 0'),
    ('icp_linearize', {'nan': ('T', 'center')}, -1, 'plade_icp_linearize: T must be finite'),
    ('icp_linearize', {'stride': 2, 'dist': 0.0}, -1, 'plade_icp_linearize: empty cloud or stride < 3'),
    ('icp_linearize', {'nan': ('center', 'tgt')}, -1, 'plade_icp_linearize: center must be finite'),
    ('refine_gicp', {'null': 'tgt'}, -1, 'plade_refine_gicp: bad argument'),
    ('refine_gicp', {'null': 'src'}, -1, 'plade_refine_gicp: bad argument'),
    ('refine_gicp', {'null': 'T'}, -1, 'plade_refine_gicp: bad argument'),
    ('refine_gicp', {'null': 'out'}, -1, 'plade_refine_gicp: bad argument'),
    ('refine_gicp', {'n_t': 0}, -1, 'plade_refine_gicp: empty cloud'),
    ('refine_gicp', {'n_s': 0}, -1, 'plade_refine_gicp: empty cloud'),
    ('refine_gicp', {'nan': ('T',)}, -1, 'refine_gicp: T_in must be finite'),
    ('refine_gicp', {'nan': ('tgt',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('refine_gicp', {'nan': ('src',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('refine_gicp', {'scene': 'one_point'}, -1, "refine_gicp: the target's bounding box is a single point"),
    ('refine_gicp', {'prm': {'source_leaf': -1.0}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp', {'prm': {'source_leaf': 'inf'}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp', {'prm': {'max_dist': -1.0}}, -1, 'refine_gicp: max_dist must be finite and >= 0'),
    ('refine_gicp', {'prm': {'max_dist': 'inf'}}, -1, 'refine_gicp: max_dist must be finite and >= 0'),
    ('refine_gicp', {'prm': {'min_dist': -1.0}}, -1, 'refine_gicp: min_dist must be finite and >= 0'),
    ('refine_gicp', {'prm': {'min_dist': 'inf'}}, -1, 'refine_gicp: min_dist must be finite and >= 0'),
    ('refine_gicp', {'prm': {'eps_rotation': -1.0}}, -1, 'refine_gicp: eps_rotation must be finite and >= 0'),
    ('refine_gicp', {'prm': {'eps_rotation': 'inf'}}, -1, 'refine_gicp: eps_rotation must be finite and >= 0'),
    ('refine_gicp', {'prm': {'eps_translation': -1.0}}, -1, 'refine_gicp: eps_translation must be finite and >= 0'),
    ('refine_gicp', {'prm': {'eps_translation': 'inf'}}, -1, 'refine_gicp: eps_translation must be finite and >= 0'),
    ('refine_gicp', {'prm': {'source_leaf': 'nan'}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp', {'prm': {'max_iterations': -1}}, -1, 'refine_gicp: max_iterations and min_correspondences must be >= 0'),
    ('refine_gicp', {'prm': {'min_correspondences': -1}}, -1, 'refine_gicp: max_iterations and min_correspondences must be >= 0'),
    ('refine_gicp', {'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, 'refine_gicp: min_dist > max_dist'),
    ('refine_gicp', {'prm': {'max_dist': 1.0, 'min_dist': 1e-06}}, -1, 'refine_gicp: more than 16 stages (max_dist / min_dist > 2^15)'),
    ('refine_gicp', {'prm': {'epsilon': -1.0}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp', {'prm': {'epsilon': 1.5}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp', {'prm': {'epsilon': 'nan'}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp', {'prm': {'source_leaf': 1e-07}}, -5, 'refine_gicp: the sample: more than 2^18 leaves along one axis'),
    ('refine_gicp', {'null': 'tgt', 'n_s': 0}, -1, 'plade_refine_gicp: bad argument'),
    ('refine_gicp', {'n_t': 0, 'nan': ('T',)}, -1, 'plade_refine_gicp: empty cloud'),
    ('refine_gicp', {'nan': ('T', 'tgt')}, -1, 'refine_gicp: T_in must be finite'),
    ('refine_gicp', {'nan': ('tgt',), 'prm': {'max_dist': -1.0}}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('refine_gicp', {'nan': ('T',), 'prm': {'max_dist': -1.0}}, -1, 'refine_gicp: T_in must be finite'),
    ('refine_gicp', {'prm': {'source_leaf': -1.0, 'max_dist': -1.0}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp', {'prm': {'eps_translation': -1.0, 'max_iterations': -1}}, -1, 'refine_gicp: eps_translation must be finite and >= 0'),
    ('refine_gicp', {'prm': {'max_iterations': -1}, 'scene': 'one_point'}, -1, 'refine_gicp: max_iterations and min_correspondences must be >= 0'),
    ('refine_gicp', {'scene': 'one_point', 'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, "refine_gicp: the target's bounding box is a single point"),
    ('refine_gicp', {'prm': {'max_dist': -1.0, 'epsilon': -1.0}}, -1, 'refine_gicp: max_dist must be finite and >= 0'),
    ('refine_gicp', {'prm': {'epsilon': -1.0, 'source_leaf': 1e-07}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp', {'scene': 'far'}, -4, 'refine_gicp: too few correspondences'),
    ('refine_gicp', {'scene': 'line', 'prm': {'min_correspondences': 10}}, -4, 'refine_gicp: degenerate geometry (the system is singular)'),
    ('refine_gicp_dev', {'null': 'tgt'}, -1, 'plade_refine_gicp_dev: bad argument'),
    ('refine_gicp_dev', {'null': 'src'}, -1, 'plade_refine_gicp_dev: bad argument'),
    ('refine_gicp_dev', {'null': 'T'}, -1, 'plade_refine_gicp_dev: bad argument'),
    ('refine_gicp_dev', {'null': 'out'}, -1, 'plade_refine_gicp_dev: bad argument'),
    ('refine_gicp_dev', {'nan': ('T',)}, -1, 'refine_gicp: T_in must be finite'),
    ('refine_gicp_dev', {'scene': 'one_point'}, -1, "refine_gicp: the target's bounding box is a single point"),
    ('refine_gicp_dev', {'prm': {'source_leaf': -1.0}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'source_leaf': 'inf'}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'max_dist': -1.0}}, -1, 'refine_gicp: max_dist must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'max_dist': 'inf'}}, -1, 'refine_gicp: max_dist must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'min_dist': -1.0}}, -1, 'refine_gicp: min_dist must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'min_dist': 'inf'}}, -1, 'refine_gicp: min_dist must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'eps_rotation': -1.0}}, -1, 'refine_gicp: eps_rotation must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'eps_rotation': 'inf'}}, -1, 'refine_gicp: eps_rotation must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'eps_translation': -1.0}}, -1, 'refine_gicp: eps_translation must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'eps_translation': 'inf'}}, -1, 'refine_gicp: eps_translation must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'source_leaf': 'nan'}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'max_iterations': -1}}, -1, 'refine_gicp: max_iterations and min_correspondences must be >= 0'),
    ('refine_gicp_dev', {'prm': {'min_correspondences': -1}}, -1, 'refine_gicp: max_iterations and min_correspondences must be >= 0'),
    ('refine_gicp_dev', {'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, 'refine_gicp: min_dist > max_dist'),
    ('refine_gicp_dev', {'prm': {'max_dist': 1.0, 'min_dist': 1e-06}}, -1, 'refine_gicp: more than 16 stages (max_dist / min_dist > 2^15)'),
    ('refine_gicp_dev', {'prm': {'epsilon': -1.0}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp_dev', {'prm': {'epsilon': 1.5}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp_dev', {'prm': {'epsilon': 'nan'}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp_dev', {'prm': {'source_leaf': 1e-07}}, -5, 'refine_gicp: the sample: more than 2^18 leaves along one axis'),
    ('refine_gicp_dev', {'null': 'src', 'nan': ('T',)}, -1, 'plade_refine_gicp_dev: bad argument'),
    ('refine_gicp_dev', {'nan': ('T',), 'prm': {'max_dist': -1.0}}, -1, 'refine_gicp: T_in must be finite'),
    ('refine_gicp_dev', {'prm': {'source_leaf': -1.0, 'max_dist': -1.0}}, -1, 'refine_gicp: source_leaf must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'eps_translation': -1.0, 'max_iterations': -1}}, -1, 'refine_gicp: eps_translation must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'max_iterations': -1}, 'scene': 'one_point'}, -1, 'refine_gicp: max_iterations and min_correspondences must be >= 0'),
    ('refine_gicp_dev', {'scene': 'one_point', 'prm': {'min_dist': 0.5, 'max_dist': 0.1}}, -1, "refine_gicp: the target's bounding box is a single point"),
    ('refine_gicp_dev', {'prm': {'max_dist': -1.0, 'epsilon': -1.0}}, -1, 'refine_gicp: max_dist must be finite and >= 0'),
    ('refine_gicp_dev', {'prm': {'epsilon': -1.0, 'source_leaf': 1e-07}}, -1, 'refine_gicp: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('refine_gicp_dev', {'scene': 'far'}, -4, 'refine_gicp: too few correspondences'),
    ('refine_gicp_dev', {'scene': 'line', 'prm': {'min_correspondences': 10}}, -4, 'refine_gicp: degenerate geometry (the system is singular)'),
    ('gicp_linearize', {'null': 'tgt'}, -1, 'plade_gicp_linearize: bad argument'),
    ('gicp_linearize', {'null': 'src'}, -1, 'plade_gicp_linearize: bad argument'),
    ('gicp_linearize', {'null': 'T'}, -1, 'plade_gicp_linearize: bad argument'),
    ('gicp_linearize', {'null': 'center'}, -1, 'plade_gicp_linearize: bad argument'),
    ('gicp_linearize', {'null': 'moments'}, -1, 'plade_gicp_linearize: bad argument'),
    ('gicp_linearize', {'n_t': 0}, -1, 'plade_gicp_linearize: empty cloud'),
    ('gicp_linearize', {'n_s': 0}, -1, 'plade_gicp_linearize: empty cloud'),
    ('gicp_linearize', {'nan': ('T',)}, -1, 'plade_gicp_linearize: T must be finite'),
    ('gicp_linearize', {'nan': ('center',)}, -1, 'plade_gicp_linearize: center must be finite'),
    ('gicp_linearize', {'nan': ('tgt',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('gicp_linearize', {'nan': ('src',)}, -1, 'the point cloud contains non-finite coordinates (NaN or infinity)'),
    ('gicp_linearize', {'dist': 0.0}, -1, 'plade_gicp_linearize: dist must be finite and > 0'),
    ('gicp_linearize', {'dist': 'inf'}, -1, 'plade_gicp_linearize: dist must be finite and > 0'),
    ('gicp_linearize', {'epsilon': -1.0}, -1, 'plade_gicp_linearize: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('gicp_linearize', {'epsilon': 1.5}, -1, 'plade_gicp_linearize: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('gicp_linearize', {'epsilon': 'nan'}, -1, 'plade_gicp_linearize: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
    ('gicp_linearize', {'null': 'center', 'n_t': 0}, -1, 'plade_gicp_linearize: bad argument'),
    ('gicp_linearize', {'n_s': 0, 'dist': 0.0}, -1, 'plade_gicp_linearize: empty cloud'),
    ('gicp_linearize', {'dist': 0.0, 'nan': ('T',)}, -1, 'plade_gicp_linearize: dist must be finite and > 0'),
    ('gicp_linearize', {'nan': ('T', 'center')}, -1, 'plade_gicp_linearize: T must be finite'),
    ('gicp_linearize', {'nan': ('center',), 'epsilon': -1.0}, -1, 'plade_gicp_linearize: center must be finite'),
    ('gicp_linearize', {'epsilon': -1.0, 'nan': ('src',)}, -1, 'plade_gicp_linearize: epsilon must be finite, 0 (the default 1e-3) or in (0, 1]'),
]
