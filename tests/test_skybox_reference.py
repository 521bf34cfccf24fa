"""The numpy reference of the skybox contract (tests/skybox_reference.py) checked on its own, without a GPU: layer order, the
s / t orientation of every face against expectations WRITTEN BY HAND from the WebGPU / Vulkan cube table, exactness on constant
cubes (edges and corners included) and the symmetry of the seamless footprint across the twelve edges."""
import itertools

import numpy as np
import pytest

import skybox_reference as sky

f32 = np.float32


def _dirs(*rows):
    return np.array(rows, dtype=f32)


def test_axis_directions_select_layers_0_to_5():
    d = _dirs((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
    face, _, _, _ = sky.select_face(d)
    assert face.tolist() == [0, 1, 2, 3, 4, 5]
    # a cube whose layer k is the colour (40 k, 0, 255 - 40 k): the axis directions read exactly their layer
    faces = np.zeros((6, 4, 4, 4), dtype=np.uint8)
    for k in range(6):
        faces[k, :, :] = (40 * k, 0, 255 - 40 * k, 255)
    got = sky.sample(faces, False, d)
    for k in range(6):
        want = np.array([f32(40 * k) / f32(255.0), 0.0, f32(255 - 40 * k) / f32(255.0), 1.0], dtype=f32)
        assert np.array_equal(got[k], want), sky.FACES[k]


# direction -> (face, column half, row half) it must land in.  By hand from the cube table of the WebGPU / Vulkan specifications
# (sc, tc per major axis): +X (-z, -y), -X (z, -y), +Y (x, z), -Y (x, -z), +Z (x, -y), -Z (-x, -y); column = s, row = t, both
# growing from 0 at the face's first texel.
QUADRANTS = [
    ((1, .5, .5), 0, 0, 0), ((1, .5, -.5), 0, 1, 0), ((1, -.5, .5), 0, 0, 1), ((1, -.5, -.5), 0, 1, 1),
    ((-1, .5, .5), 1, 1, 0), ((-1, .5, -.5), 1, 0, 0), ((-1, -.5, .5), 1, 1, 1), ((-1, -.5, -.5), 1, 0, 1),
    ((.5, 1, .5), 2, 1, 1), ((-.5, 1, .5), 2, 0, 1), ((.5, 1, -.5), 2, 1, 0), ((-.5, 1, -.5), 2, 0, 0),
    ((.5, -1, .5), 3, 1, 0), ((-.5, -1, .5), 3, 0, 0), ((.5, -1, -.5), 3, 1, 1), ((-.5, -1, -.5), 3, 0, 1),
    ((.5, .5, 1), 4, 1, 0), ((-.5, .5, 1), 4, 0, 0), ((.5, -.5, 1), 4, 1, 1), ((-.5, -.5, 1), 4, 0, 1),
    ((.5, .5, -1), 5, 0, 0), ((-.5, .5, -1), 5, 1, 0), ((.5, -.5, -1), 5, 0, 1), ((-.5, -.5, -1), 5, 1, 1),
]


@pytest.mark.parametrize("srgb", [False, True])
def test_quadrant_orientation_of_every_face(srgb):
    n = 8
    colours = {(0, 0): (255, 0, 0), (1, 0): (0, 255, 0), (0, 1): (0, 0, 255), (1, 1): (255, 255, 0)}  # (column half, row half)
    faces = np.zeros((6, n, n, 4), dtype=np.uint8)
    for (ch, rh), col in colours.items():
        faces[:, rh * 4:rh * 4 + 4, ch * 4:ch * 4 + 4, :3] = col
    faces[..., 3] = 255
    for d, face, ch, rh in QUADRANTS:
        assert int(sky.select_face(_dirs(d))[0][0]) == face, d
        got = sky.sample(faces, srgb, _dirs(d))[0]
        # the direction hits the middle of a quadrant: its footprint stays inside it, the value is that colour exactly
        assert got.tolist() == [c / 255 for c in colours[(ch, rh)]] + [1.0], (d, sky.FACES[face])


def _sphere_dirs(count, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((count, 3)).astype(f32)
    return d


def _edge_and_corner_dirs():
    out = []
    for sx, sy, sz in itertools.product((-1, 1), repeat=3):
        out.append((sx, sy, sz))                       # the eight corners, exactly
        for e in (1e-3, 1e-6):
            out += [(sx * (1 - e), sy, sz), (sx, sy * (1 - e), sz), (sx, sy, sz * (1 - e))]
    for a, b in itertools.combinations(range(3), 2):   # the twelve edges, exactly and just off
        for sa, sb in itertools.product((-1, 1), repeat=2):
            for third in (-0.9, -0.31, 0.0, 0.47, 0.99):
                for e in (0.0, 1e-4):
                    v = [0.0, 0.0, 0.0]
                    v[a], v[b], v[3 - a - b] = sa, sb * (1 - e), third
                    out.append(tuple(v))
    return np.array(out, dtype=f32)


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_constant_cubes_sample_to_exactly_their_colour(n, srgb):
    """every channel byte 0 or 255: the decoded texels are 0.0 / 1.0, c * (1 - f) + c * f is exact for them and so is
    ((c + c) + c) / 3 -- any direction, edges and corners included, returns the colour itself"""
    d = np.concatenate([_sphere_dirs(2000, 7 * n + srgb), _edge_and_corner_dirs()])
    for col in ((255, 0, 0), (0, 255, 255), (255, 255, 255), (0, 0, 0), (255, 0, 255)):
        faces = np.zeros((6, n, n, 4), dtype=np.uint8)
        faces[..., :3] = col
        faces[..., 3] = 77  # the cube's alpha is not sampled
        got = sky.sample(faces, srgb, d)
        want = np.array([c / 255 for c in col] + [1.0], dtype=f32)
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), col


def test_mirrored_directions_across_each_edge_read_the_same_texels():
    """the plane through an edge and the cube's centre mirrors one face onto its neighbour; a direction near the edge and its
    mirror image must read the same four texels (two of each face), whichever side evaluates the footprint"""
    n = 7
    rng = np.random.default_rng(12)
    edges = 0
    for a, b in itertools.combinations(range(3), 2):
        for sa, sb in itertools.product((-1, 1), repeat=2):
            edges += 1
            for _ in range(40):
                third = rng.uniform(-0.8, 0.8)   # away from the corners
                v = np.zeros(3)
                v[a], v[b], v[3 - a - b] = sa, sb * (1.0 - rng.uniform(0.0, 0.9 / n)), third  # inside the last half texel of face a
                m = v.copy()
                m[a], m[b] = sa * sb * v[b], sa * sb * v[a]  # reflection that swaps the two faces
                fa, fb = sky.footprint_texels(v, n), sky.footprint_texels(m, n)
                assert int(sky.select_face(v.astype(f32)[None])[0][0]) != int(sky.select_face(m.astype(f32)[None])[0][0])
                assert fa == fb and len(fa) == 4, (v, m, fa, fb)
                assert len({t[0] for t in fa}) == 2
    assert edges == 12


def test_corner_footprint_reads_three_faces():
    n = 4
    t = sky.footprint_texels(np.array([1.0, 0.999, 0.998]), n)
    assert {f for f, _, _ in t} == {0, 2, 4}


def test_takes_sky_follows_greater_equal():
    assert sky.takes_sky([0.0, -0.0, 1e-30, 0.5, np.nan]).tolist() == [True, True, False, False, False]
