"""Non-rectangular test geometries (axis-parallel polygons, clockwise like the reference's
rectangle, Grid.cpp:28-72) shared by the CPU and GPU mask tests: vertices, x / y segment
specs (Grid.cpp:78-120 format: start, end, cells, ratio) and one (type, info) BC per edge."""
INLET, WALL, NEUMANN = 0, 2, 4

# backward-facing step: inlet on the upper half of x = 0, outflow at x = 2
STEP = dict(vertices=[(0, 0.5), (0, 1), (2, 1), (2, 0), (0.5, 0), (0.5, 0.5)],
            xspec=[[0, 2, 48, -1]], yspec=[[0, 1, 24, -1]],
            bc=[(INLET, 1.0), (WALL, 0.0), (NEUMANN, 0.0), (WALL, 0.0), (WALL, 0.0), (WALL, 0.0)])
# L-shaped lid-driven cavity (the lid is the top edge)
LSHAPE = dict(vertices=[(0, 0), (0, 1), (1, 1), (1, 0.5), (0.5, 0.5), (0.5, 0)],
              xspec=[[0, 1, 32, -1]], yspec=[[0, 1, 32, -1]],
              bc=[(WALL, 0.0), (WALL, 1.0), (WALL, 0.0), (WALL, 0.0), (WALL, 0.0), (WALL, 0.0)])
# a rectangle whose west side is two edges (inlet below, wall above): every cell inside, but
# not the four-edge rectangle of the fast path
SPLIT = dict(vertices=[(0, 0), (0, 0.5), (0, 1), (1, 1), (1, 0)],
             xspec=[[0, 1, 24, -1]], yspec=[[0, 1, 20, -1]],
             bc=[(INLET, 0.5), (WALL, 0.0), (WALL, 1.0), (NEUMANN, 0.0), (WALL, 0.0)])
# a stretched U-channel: inlet bottom-left, outflow bottom-right, around a central block
UCHAN = dict(vertices=[(0, 0), (0, 1), (1.5, 1), (1.5, 0), (1, 0), (1, 0.5), (0.5, 0.5), (0.5, 0)],
             xspec=[[0, 0.5, 10, 1.05], [0.5, 1.0, 12, -1], [1.0, 1.5, 10, 0.95]], yspec=[[0, 1, 24, -1]],
             bc=[(WALL, 0.0), (WALL, 0.0), (WALL, 0.0), (WALL, 0.0), (NEUMANN, 0.0), (WALL, 0.0), (WALL, 0.0),
                 (INLET, 1.0)])
# the L-shaped cavity on a stretched grid (walls only: the area-consistent Poisson rhs)
LSHAPE_S = dict(LSHAPE, xspec=[[0, 0.5, 12, 1.04], [0.5, 1, 12, 0.96]], yspec=[[0, 0.5, 10, 0.95], [0.5, 1, 14, -1]])
# (r5) the backward-facing step on a power-of-two box (64 x 32): its bounding box has the direct solve with the
# outflow elimination, so the GPU's Poisson solve is the bordered capacitance solve
STEP_P2 = dict(STEP, xspec=[[0, 2, 64, -1]], yspec=[[0, 1, 32, -1]])
ALL = {"step": STEP, "lshape": LSHAPE, "split": SPLIT, "uchannel": UCHAN, "lshape_s": LSHAPE_S, "step_p2": STEP_P2}
# (r6) larger boxes for the masked LDS-tiled kernels (64-column tiles, 2-cell ring in j): ny >= 128, so checked
# comparisons cross the column-tile boundaries; not in ALL (the per-kernel sets stay small)
LSHAPE_BIG = dict(LSHAPE, xspec=[[0, 1, 160, -1]], yspec=[[0, 1, 200, -1]])
STEP_BIG = dict(STEP, xspec=[[0, 2, 256, -1]], yspec=[[0, 1, 136, -1]])
BIG = {"lshape_big": LSHAPE_BIG, "step_big": STEP_BIG}


def _cells(verts, nx, ny, bc):
    """Uniform hx = hy = 1 / ny on an nx x ny box; vertices given in cells."""
    return dict(vertices=[(x / ny, y / ny) for x, y in verts], xspec=[[0, nx / ny, nx, -1]], yspec=[[0, 1, ny, -1]],
                bc=[bc.get(k, (WALL, 0.0)) for k in range(len(verts))])


# Narrow features (2-cell arms and throats, a 1-cell divider) and bounding boxes whose outside region falls into
# several connected components (plus 4; dumbbell, tee, tee_hxhy, throat_out 2; u_div1, stairs 1).  Not in ALL / BIG
# (their parametrised sets stay as they are).  bc: edge index (0-based, from vertex k to k + 1) -> (type, info)
_TEE = [(6, 0), (6, 10), (0, 10), (0, 16), (16, 16), (16, 10), (10, 10), (10, 0)]
NARROW = {
    # 60 cells, none FC_DEEP; the lid is the top of the upper arm
    "plus": _cells([(7, 0), (7, 7), (0, 7), (0, 9), (7, 9), (7, 16), (9, 16), (9, 9), (16, 9), (16, 7), (9, 7), (9, 0)],
                   16, 16, {5: (WALL, 1.0)}),
    # two 8 x 16 lobes joined by a 2-cell throat, lids 1.0 and -0.5
    "dumbbell": _cells([(0, 0), (0, 16), (8, 16), (8, 9), (16, 9), (16, 16), (24, 16), (24, 0), (16, 0), (16, 7),
                        (8, 7), (8, 0)], 24, 16, {1: (WALL, 1.0), 5: (WALL, -0.5)}),
    "tee": _cells(_TEE, 16, 16, {3: (WALL, 1.0)}),
    # the tee on lx = 0.5: hx = hy / 2, unequal face weights, a non-symmetric capacitance matrix
    "tee_hxhy": dict(_cells(_TEE, 16, 16, {3: (WALL, 1.0)}), vertices=[(x / 32, y / 16) for x, y in _TEE],
                     xspec=[[0, 0.5, 16, -1]]),
    # two arms either side of a divider one cell thick
    "u_div1": _cells([(0, 0), (0, 16), (9, 16), (9, 6), (10, 6), (10, 16), (20, 16), (20, 0)], 20, 16,
                     {1: (WALL, 1.0), 5: (WALL, 0.5)}),
    "stairs": _cells([(0, 0), (0, 16), (16, 16), (16, 12), (12, 12), (12, 8), (8, 8), (8, 4), (4, 4), (4, 0)], 16, 16,
                     {1: (WALL, 1.0)}),
    # a channel with a 2-cell constriction: inlet W, outflow on the box's whole E column (the bordered system)
    "throat_out": _cells([(0, 0), (0, 16), (12, 16), (12, 9), (20, 9), (20, 16), (32, 16), (32, 0), (20, 0), (20, 7),
                          (12, 7), (12, 0)], 32, 16, {0: (INLET, 0.25), 6: (NEUMANN, 0.0)}),
}
# outside components of each NARROW shape's bounding box (4-connected)
NARROW_COMPONENTS = {"plus": 4, "dumbbell": 2, "tee": 2, "tee_hxhy": 2, "u_div1": 1, "stairs": 1, "throat_out": 2}
# SPLIT's five-vertex form (the W side as two wall edges, a lid on top) on tiny boxes: the masked path with every
# cell in the domain and no interface face
SPLITS = {f"split_{nx}x{ny}": _cells([(0, 0), (0, ny // 2), (0, ny), (nx, ny), (nx, 0)], nx, ny, {2: (WALL, 1.0)})
          for nx, ny in ((2, 2), (3, 4), (4, 3), (5, 5))}
# 1024 columns: the masked inverse transform of the capacitance solve (ny = 1024 ... 8192)
NARROW_TALL = {
    "lshape_1024": _cells([(0, 0), (0, 1024), (24, 1024), (24, 512), (12, 512), (12, 0)], 24, 1024, {1: (WALL, 1.0)}),
    "tee_1024": _cells([(6, 0), (6, 640), (0, 640), (0, 1024), (16, 1024), (16, 640), (10, 640), (10, 0)], 16, 1024,
                       {3: (WALL, 1.0)}),
}
