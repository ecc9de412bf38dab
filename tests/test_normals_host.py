"""Clouds without normals, host side (no GPU): the entry points of normal estimation are exported, and plade_ply_read_points
reads xyz-only PLY files (NaN normal columns, has_normals = 0) while it agrees with plade_ply_read on everything else."""
import os

import numpy as np
import pytest

import plade_amd

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "ply_cases.npz"))
NAMES = [str(n) for n in GOLD["names"]]
MISSING_NORMALS = {"no_normals_fails", "normals_incomplete_fails"}   # the only failures read_ply_points accepts


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def test_new_symbols_are_exported():
    L = plade_amd.load_library()
    for s in ("plade_estimate_normals", "plade_cloud_upload_xyz", "plade_ply_read_points"):
        assert hasattr(L, s), s
        assert s in plade_amd.ABI_SYMBOLS
    assert callable(plade_amd.read_ply_points)
    assert callable(plade_amd.Context.estimate_normals) and callable(plade_amd.Context.upload_xyz)


def _xyz(n=257, seed=3, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * rng.uniform(0.1, 100.0, size=(n, 1))).astype(dtype)


def _write(path, xyz, mode, dtype, extra=False):
    t = "float" if dtype == np.float32 else "double"
    props = [f"property {t} x", f"property {t} y", f"property {t} z"]
    if extra:
        props.insert(1, "property uchar red")
    head = f"ply\nformat {mode} 1.0\ncomment xyz only\nelement vertex {len(xyz)}\n" + "\n".join(props) + "\nend_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        if mode == "ascii":
            for p in xyz:
                vals = [repr(float(v)) if dtype == np.float64 else repr(float(np.float32(v))) for v in p]
                if extra:
                    vals.insert(1, "7")
                f.write((" ".join(vals) + "\n").encode())
        else:
            end = "<" if mode == "binary_little_endian" else ">"
            fields = [("x", end + ("f4" if dtype == np.float32 else "f8")), ("y", end + ("f4" if dtype == np.float32 else "f8")),
                      ("z", end + ("f4" if dtype == np.float32 else "f8"))]
            if extra:
                fields.insert(1, ("red", "u1"))
            rec = np.zeros(len(xyz), dtype=fields)
            rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            if extra:
                rec["red"] = 7
            f.write(rec.tobytes())


@pytest.mark.parametrize("mode", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("extra", [False, True])
def test_xyz_only_files_read_exactly(tmp_path, mode, dtype, extra):
    xyz = _xyz(dtype=dtype)
    path = str(tmp_path / "pts.ply")
    _write(path, xyz, mode, dtype, extra)
    a, has = plade_amd.read_ply_points(path)
    assert has is False
    assert a.shape == (len(xyz), 6) and a.dtype == np.float32
    assert _same_bits(a[:, :3], xyz.astype(np.float64).astype(np.float32))      # every value through double to float
    assert np.isnan(a[:, 3:]).all()
    with pytest.raises(plade_amd.PladeError) as e:                                 # plade_ply_read itself is unchanged
        plade_amd.read_ply(path)
    assert "the number of points does not equal to the number of normals" in str(e.value)


@pytest.mark.parametrize("name", NAMES)
def test_golden_cases_agree_with_read_ply(tmp_path, name):
    path = str(tmp_path / "case.ply")
    with open(path, "wb") as f:
        f.write(GOLD["file_" + name].tobytes())
    if bool(GOLD["ok_" + name]):
        a, has = plade_amd.read_ply_points(path)
        assert has is True
        assert _same_bits(a, plade_amd.read_ply(path))
        return
    with pytest.raises(plade_amd.PladeError) as want:
        plade_amd.read_ply(path)
    if name in MISSING_NORMALS:
        a, has = plade_amd.read_ply_points(path)
        assert has is False and len(a) > 0 and np.isnan(a[:, 3:]).all() and np.isfinite(a[:, :3]).all()
        return
    with pytest.raises(plade_amd.PladeError) as got:
        plade_amd.read_ply_points(path)
    assert str(got.value) == str(want.value)


def test_missing_file_message_is_read_plys(tmp_path):
    p = str(tmp_path / "nope.ply")
    with pytest.raises(plade_amd.PladeError) as a:
        plade_amd.read_ply(p)
    with pytest.raises(plade_amd.PladeError) as b:
        plade_amd.read_ply_points(p)
    assert str(a.value) == str(b.value)


CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plade_amd", "PLADE")
# what the CLI of the parent revision prints and records for a pair of xyz-only PLY files (the load fails before any GPU work)
PARENT_STDOUT = "target file: {t}\nsource file: {s}\n"
PARENT_STDERR = "the number of points does not equal to the number of normals in the file\nloading target point cloud failed\n"
PARENT_RESULT = "registration failed, an identity matrix is recorded:\n1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n"


def test_cli_without_the_switch_fails_as_before_and_with_it_accepts_the_file(tmp_path):
    import subprocess
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    for p, seed in ((pt, 1), (ps, 2)):
        _write(p, _xyz(100, seed=seed), "binary_little_endian", np.float32)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    for extra in ({}, {"PLADE_ESTIMATE_NORMALS": "0"}):
        res = str(tmp_path / "r.txt")
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert (r.returncode, r.stdout, r.stderr) == (1, PARENT_STDOUT.format(t=pt, s=ps), PARENT_STDERR), extra
        assert open(res).read() == PARENT_RESULT
    # with the switch the files are accepted (what follows needs a GPU: estimated and registered, or a context error)
    r = subprocess.run([CLI, pt, ps, str(tmp_path / "r1.txt")], capture_output=True, text=True, timeout=300,
                       env=dict(env, PLADE_ESTIMATE_NORMALS="16"))
    assert "the number of points does not equal to the number of normals" not in r.stderr
