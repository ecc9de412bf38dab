#!/usr/bin/env python3
"""tests/golden/ply_fuzz.npz -- the REFERENCE's verdicts on the random PLY files of tests/test_ply_fuzz.py (default seed).

Per file: status 1 (accepted), 0 (refused) or -1 (the reference's process died on it), the point count and the SHA-256 of the
returned floats (NaNs zeroed, NaN mask appended), as tests/ply_ref_helper.py prints them; plus the SHA-256 of all the files, so
that a change of the generator is caught.  Needs oracle/_ref (built where the reference tree exists).
Run: python tools/make_golden_ply_fuzz.py"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ply_fuzz as fz  # noqa: E402


def main():
    import tempfile
    files = fz.random_files(fz.DEFAULT_SEED)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k, data in enumerate(files):
            paths.append(os.path.join(d, f"f{k}.ply"))
            with open(paths[-1], "wb") as f:
                f.write(data)
        ref = fz.reference_verdicts(paths)
    status = np.array([-1 if v == "died" else int(v[0]) for v in ref], np.int8)
    n = np.array([0 if v == "died" else v[1] for v in ref], np.int64)
    sha = np.array(["-" if v == "died" else v[2] for v in ref])
    np.savez_compressed(fz.GOLDEN, status=status, n=n, sha256=sha, seed=np.int64(fz.DEFAULT_SEED),
                        files_sha256=np.array(hashlib.sha256(b"".join(files)).hexdigest()))
    print(f"{fz.GOLDEN}: {int((status == 1).sum())} accepted, {int((status == 0).sum())} refused, {int((status < 0).sum())} died")


if __name__ == "__main__":
    main()
