"""The inputs of the ISS keypoint tests (test_iss_host.py, test_gpu_iss.py and the CLI / C++ tests) and their restated answers,
computed once per process (tests/iss_restate.py is a brute force over all pairs: about a second per 6000-point case)."""
import functools

import numpy as np

import corr_cases
import iss_restate as I
from plade_amd.synth import sample_scene

F32 = np.float32
SCENE_D = 13.2                      # the diagonal of the room of sample_scene
TIE_PAIR, TIE_LONELY = (6, 7), 8
# the end-to-end run on the terrain pair: FPFH radius, salient and non-max radius, inlier distance
TERRAIN = dict(radius=0.6, salient_radius=0.5, non_max_radius=0.15, inlier_dist=0.1)


def cubic_lattice():
    """8 x 8 x 8 points of pitch 2^-3"""
    g = np.arange(8, dtype=F32) * F32(0.125)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))


def planar_lattice():
    """32 x 32 points of pitch 2^-5 at z = 0.5"""
    g = np.arange(32, dtype=F32) * F32(2.0 ** -5)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), np.full(1024, 0.5, F32)], axis=1))


def point_row():
    """64 points of pitch 2^-5 along x"""
    P = np.zeros((64, 3), F32)
    P[:, 0] = np.arange(64, dtype=F32) * F32(2.0 ** -5)
    P[:, 1:] = (0.25, -0.75)
    return P


def tie_cloud():
    """six points on the axes around a coincident pair at the origin (rows TIE_PAIR), and a pair of points far away whose
    neighbourhoods within 1.0 hold two points each (row TIE_LONELY and the next)"""
    return np.array([[0.875, 0, 0], [-0.875, 0, 0], [0, 0.75, 0], [0, -0.75, 0], [0, 0, 0.5625], [0, 0, -0.5625],
                     [0, 0, 0], [0, 0, 0], [10, 10, 10], [10.5, 10, 10]], F32)


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(n, 6) float32: "scene" = sample_scene(6000, scene_seed=3, sample_seed=4), "terrain" = the source of terrain_pair(6000)"""
    if name == "scene":
        c = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=4), F32)
    else:
        c = terrain()[1]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def terrain():
    """(target, source, T) of corr_cases.terrain_pair(6000)"""
    tg, sr, T = corr_cases.terrain_pair(6000)
    tg.setflags(write=False); sr.setflags(write=False)
    return tg, sr, T


def gpu_cases():
    """(name, cloud, salient_radius, non_max_radius, gamma) of the four inputs of the GPU tests"""
    return [("scene", cloud("scene"), 0.04 * SCENE_D, 0.04 * SCENE_D, 0.975), ("scene", cloud("scene"), 0.08 * SCENE_D, 0.04 * SCENE_D, 0.6),
            ("terrain", cloud("terrain"), 0.5, 0.15, 0.975), ("terrain", cloud("terrain"), 0.5, 0.15, 0.6)]


@functools.lru_cache(maxsize=None)
def restated(name, salient_radius, non_max_radius, gamma):
    """iss_restate.iss of cloud(name) with gamma21 = gamma32 = gamma and the default min_neighbours"""
    return I.iss(cloud(name), salient_radius, non_max_radius, gamma, gamma)
