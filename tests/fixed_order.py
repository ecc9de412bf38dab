"""The fixed order of the cloud tools' summary reductions (plade_amd/csrc/fixed_reduce.h), replayed in numpy.

The library is built with -ffp-contract=off, so the same operations in the same order give the same bits: workgroups of 256
values (lanes past the end hold 0), per 64-lane wave the xor butterfly v = op(v, v[lane ^ o]) for o = 32 .. 1 (lane 0's value),
the four waves combined in ascending order; then one wavefront whose lane l starts from 0 and takes the workgroups' partials
l, l + 64, ... in ascending order, and the butterfly again."""
import numpy as np

_LANE = np.arange(64)


def _butterfly(v, op):
    """v: (..., 64) -> lane 0's value after the butterfly, (...)"""
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., _LANE ^ o])
    return v[..., 0]


def reduce(values, op):
    """values: a 1-d array (n >= 1) of the per-point terms; op: np.add, np.fmax (doubles) or np.maximum (integers)."""
    v = np.asarray(values)
    n = len(v)
    blocks = -(-n // 256)
    lanes = np.zeros(blocks * 256, v.dtype)
    lanes[:n] = v
    waves = _butterfly(lanes.reshape(blocks, 4, 64), op)
    partial = waves[:, 0]
    for w in range(1, 4):
        partial = op(partial, waves[:, w])
    acc = np.zeros(64, v.dtype)
    for b0 in range(0, blocks, 64):
        take = partial[b0:b0 + 64]
        acc[:len(take)] = op(acc[:len(take)], take)
    return _butterfly(acc, op)[()]
