"""The numpy model of the ground layer (tests/ground_model.py) on hand-made columns whose answer is written out here: what the rules
of ws_map_ground in include/warpsense_hip.h say, read by a person.  No GPU."""
import numpy as np

import ground_model as G

U, F, O = 0, 1, 2
T = G.TAU


def col(cls, values, H, lo_z=10, **kw):
    return G.column(list(cls), list(values), lo_z, H, **kw)


def test_a_floor():
    #        z = 10  11   12  13  14  15
    cls = (O, O, F, F, F, F)
    val = (-T, -200, 600, T, T, T)
    # the level is z = 11: occupied under free, headroom 12 .. 14 for H = 3; frac = floor(256 * 200 / 800) = 64
    assert col(cls, val, 3) == (G.GROUND, 11, 64)
    assert col(cls, val, 4) == (G.GROUND, 11, 64)       # z + H = 15 is the last voxel of the box
    assert col(cls, val, 5) == (G.BLOCKED, 0, 0)        # z + H = 16 lies outside the box
    assert col(cls, val, 1, top=True) == (G.GROUND, 11, 64)


def test_a_floor_under_a_table():
    #      10  11 12 13 14  15 16 17 18
    cls = (O, F, F, F, O, F, F, F, F)
    val = (-100, 100, T, T, -50, 150, T, T, T)
    assert col(cls, val, 2) == (G.GROUND, 10, 128)               # the lowest: the floor, 256 * 100 / 200
    assert col(cls, val, 2, top=True) == (G.GROUND, 14, 64)      # the highest: the table, 256 * 50 / 200
    assert col(cls, val, 3) == (G.GROUND, 10, 128)               # the floor has 11 .. 13 free
    assert col(cls, val, 4) == (G.GROUND, 14, 64)                # under the table only 3 voxels are free: the table top is the one level
    assert col(cls, val, 5) == (G.BLOCKED, 0, 0)                 # 14 + 5 lies outside the box


def test_a_ceiling_only():
    # FREE below OCCUPIED is no level: nothing to stand on, and the column holds an occupied voxel
    assert col((F, F, F, O, O), (T, T, 100, -100, -T), 1) == (G.BLOCKED, 0, 0)
    # the top voxel of the box is occupied with nothing above it inside the box
    assert col((F, F, F, F, O), (T, T, T, 100, -100), 1) == (G.BLOCKED, 0, 0)


def test_headroom_one_voxel_short():
    cls = (O, F, F, F, U, F, F)
    val = (-300, 300, T, T, 0, T, T)
    assert col(cls, val, 3) == (G.GROUND, 10, 128)
    assert col(cls, val, 4) == (G.BLOCKED, 0, 0)                            # z + 4 is unknown
    assert col(cls, val, 4, unknown_headroom=True) == (G.GROUND, 10, 128)   # ... which UNKNOWN_HEADROOM accepts
    assert col(cls, val, 6, unknown_headroom=True) == (G.GROUND, 10, 128)
    assert col(cls, val, 7, unknown_headroom=True) == (G.BLOCKED, 0, 0)     # z + 7 lies outside the box
    # z + 1 must be FREE in every case: the height needs its value
    assert col((O, U, F, F), (-300, 0, T, T), 2, unknown_headroom=True) == (G.BLOCKED, 0, 0)
    # an occupied voxel in the headroom is never accepted
    assert col((O, F, O, F, F), (-300, 300, -5, 5, T), 2, unknown_headroom=True) == (G.GROUND, 12, 128)


def test_v1_zero_clamps_frac():
    assert G.frac_of(-1, 0) == 255 and G.frac_of(-32768, 0) == 255     # 256 clamps to 255
    assert G.frac_of(-1, 32767) == 0 and G.frac_of(-32768, 32767) == 128 and G.frac_of(-1, 1) == 128 and G.frac_of(-255, 1) == 255
    assert col((O, F, F), (-7, 0, T), 1) == (G.GROUND, 10, 255)


def test_void_and_unknown():
    assert col((F, F, F), (T, T, T), 1) == (G.VOID, 0, 0)          # a hole: seen, and nothing to stand on
    assert col((U, F, U), (0, T, 0), 1) == (G.VOID, 0, 0)
    assert col((U, U, U), (0, 0, 0), 1) == (G.UNKNOWN, 0, 0)
    assert col((O,), (-5,), 1) == (G.BLOCKED, 0, 0)                # a box one voxel high never holds a level


def ramp_box():
    """9 x 3 columns over z = 0 .. 19 (lo = (0, 0, 0)): a ramp of one voxel per column in x, the same in every y; column x has its
    floor at z = 2 + x with v0 = -(100 + 20 x), v1 = 300, so frac = floor(256 (100 + 20 x) / (400 + 20 x))"""
    value, weight = G.entries((9, 3, 20))
    for x in range(9):
        for y in range(3):
            G.put_floor(value, weight, x, y, 2 + x, v0=-(100 + 20 * x), v1=300, free=6)
    return G.pack(value, weight)


def test_a_ramp():
    rec, counts = G.model_box(ramp_box(), (0, 0, 0), 4)
    assert counts.tolist() == [0, 27, 0, 0]
    frac = [(256 * (100 + 20 * x)) // (400 + 20 * x) for x in range(9)]
    assert frac == [64, 73, 81, 89, 96, 102, 108, 113, 118]
    for x in range(9):
        assert np.all(rec["z"][x] == 2 + x) and np.all((rec["w"][x] & 0xFF) == frac[x]) and np.all(rec["w"][x] >> 30 == G.GROUND)
        # the step is 256 +- the frac differences: to x + 1 it is 256 + frac[x + 1] - frac[x], to x - 1 it is 256 + frac[x] - frac[x - 1]
        want = max(([256 + frac[x + 1] - frac[x]] if x < 8 else []) + ([256 + frac[x] - frac[x - 1]] if x > 0 else []))
        assert np.all(((rec["w"][x] >> 8) & 0xFFFF) == want), (x, want)
    assert ((int(rec["w"][0, 0]) >> 8) & 0xFFFF) == 265 and ((int(rec["w"][8, 1]) >> 8) & 0xFFFF) == 261
    # every column is FREE for a robot that climbs 265/256 voxel, and the first one is a site for one that climbs 264
    assert np.all(G.bridge_classes(rec, 265) == 1)
    cls = G.bridge_classes(rec, 264)
    assert np.all(cls[0] == 2) and np.all(cls[1] == 2) and np.all(cls[8] == 1)


def kerb_box():
    """6 x 2 columns: a floor at z = 3 for x < 3, a kerb of two voxels, a floor at z = 5 for x >= 3; the same values everywhere"""
    value, weight = G.entries((6, 2, 16))
    for x in range(6):
        for y in range(2):
            G.put_floor(value, weight, x, y, 3 if x < 3 else 5, free=6)
            if x >= 3:
                value[x, y, 3:5], weight[x, y, 3:5] = -G.TAU, 5  # the kerb is solid
    return G.pack(value, weight)


def test_a_kerb():
    rec, counts = G.model_box(kerb_box(), (0, 0, 0), 4)
    assert counts.tolist() == [0, 12, 0, 0]
    step = (rec["w"] >> 8) & 0xFFFF
    assert step[:2].max() == 0 and step[4:].max() == 0 and np.all(step[2:4] == 512)   # two voxels, the same frac on both sides
    assert np.all(G.bridge_classes(rec, 256)[2:4] == 2) and np.all(G.bridge_classes(rec, 768) == 1)
    d, sites = G.bridge_model(rec, 256, 3)
    assert sites == 4 and np.array_equal(d[:, 0] & 0xFFFFFF, [4, 1, 0, 0, 1, 4])
    d, sites = G.bridge_model(rec, 768, 3)
    assert sites == 0 and np.all(d == ((1 << 30) | 9))


def test_a_hole_and_a_wall():
    value, weight = G.entries((3, 3, 10))
    for x in range(3):
        for y in range(3):
            G.put_floor(value, weight, x, y, 2, free=5)
    value[1, 1, :], weight[1, 1, :] = G.TAU, 5        # a hole: free all the way down
    value[0, 2, :], weight[0, 2, :] = -G.TAU, 5       # a wall: occupied all the way up
    weight[2, 0, :] = 0                                # never seen
    weight[2, 2, :] = -5                               # negative weights: unknown unless ANY_WEIGHT
    rec, counts = G.model_box(G.pack(value, weight), (5, 6, -7), 3)
    kind = rec["w"] >> 30
    assert kind[1, 1] == G.VOID and kind[0, 2] == G.BLOCKED and kind[2, 0] == G.UNKNOWN and kind[2, 2] == G.UNKNOWN and counts.tolist() == [2, 5, 1, 1]
    assert rec["z"][0, 0] == -5 and rec["z"][1, 1] == 0 and np.all(((rec["w"] >> 8) & 0xFFFF) == 0)   # the floor is level around the hole
    assert G.bridge_classes(rec, 65535).tolist() == [[1, 1, 2], [1, 2, 1], [0, 1, 0]]
    rec, counts = G.model_box(G.pack(value, weight), (5, 6, -7), 3, any_weight=True)
    assert (rec["w"] >> 30)[2, 2] == G.GROUND and counts.tolist() == [1, 6, 1, 1]
