#!/usr/bin/env python3
"""Generates mipsfusion_amd/csrc/mcubes_tables.h: the 256-case triangle table of the mesh extractor.

Nothing here is copied from a published table.  For every sign pattern of the eight cell corners the iso-lines on the six
cube faces are traced, joined into closed loops and each loop is cut into a triangle fan:

* corner ``c = 4*dx + 2*dy + dz`` (dx, dy, dz in {0, 1}); bit ``c`` of the case is set when ``value[c] < isovalue``;
* edge ``e``: 0-3 run along x at (dy, dz) = (0,0) (0,1) (1,0) (1,1), 4-7 along y at (dx, dz) likewise, 8-11 along z at
  (dx, dy) likewise.  ``EDGE_ENDS[e] = (first, second)`` is the direction in which the vertex is interpolated
  (``first + mu * (second - first)``).  It only shows where a vertex snaps to an end point, and is chosen so that the snapped
  planes of the fixtures ``plane_snap`` / ``plane_snap2`` come out where the recorded meshes have them: x edges run towards
  +x at dy = 1 and towards -x at dy = 0, y edges towards +y at dx = 0 and towards -y at dx = 1, z edges towards +z;
* a face with two crossed edges holds one segment; a face whose corner signs alternate holds two, and ONE rule decides how
  it is cut (``FACE_RULE``): "separate" cuts each below-isovalue corner off on its own, "join" connects the two
  below-isovalue corners across the face (cutting each above-isovalue corner off);
* segments are directed with the below-isovalue side on their left seen from outside the cube, which makes every crossed edge
  the end of one segment and the start of another, so the segments chain into closed loops;
* a loop is fanned from one of its vertices: (l0, l1, l2), (l0, l2, l3), ... or, with ``FLIP``, (l0, l2, l1), ...  The fan
  starts at the smallest edge number for which no triangle has its three vertices on one face of the cube (such a triangle
  would lie in the face, where the neighbouring cell may produce it again); loops are taken in the order of their smallest
  edge.

``FACE_RULE`` and ``FLIP`` are decided by the recorded behaviour in tests/golden/mcubes_cases.npz (tests/test_mcubes_cpu.py
compares the vector area of every case, which depends on the loops and their winding and not on the fan).
``EXCEPTIONS`` lists cases whose recorded loops are not what the one face rule gives (own edge numbering).

usage: tools/gen_mcubes_tables.py [--check] [-o FILE]
"""
import argparse
import os
import sys

import numpy as np

FACE_RULE = "separate"
FLIP = True
# case -> list of loops (edge numbers, directed as described above) replacing what the face rule gives.
# Recorded: the two patterns in which all eight x and y edges are crossed and no z edge is (corners 2 3 4 5 below the isovalue,
# or above it: two z edges diagonally opposite) emit nothing upstream.  The face rule would give two quads.
EXCEPTIONS = {60: [], 195: []}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mipsfusion_amd", "csrc", "mcubes_tables.h")
MAX_TRIS = 5

CORNERS = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], dtype=np.float64)


def _corner(dx, dy, dz):
    return 4 * dx + 2 * dy + dz


def _edge_ends():
    ends = []
    for dy in (0, 1):
        for dz in (0, 1):
            a, b = _corner(0, dy, dz), _corner(1, dy, dz)
            ends.append((a, b) if dy == 1 else (b, a))
    for dx in (0, 1):
        for dz in (0, 1):
            a, b = _corner(dx, 0, dz), _corner(dx, 1, dz)
            ends.append((a, b) if dx == 0 else (b, a))
    for dx in (0, 1):
        for dy in (0, 1):
            ends.append((_corner(dx, dy, 0), _corner(dx, dy, 1)))
    return ends


EDGE_ENDS = _edge_ends()
EDGE_OF = {frozenset(e): i for i, e in enumerate(EDGE_ENDS)}
EDGE_MID = np.array([(CORNERS[a] + CORNERS[b]) / 2 for a, b in EDGE_ENDS])


def _faces():
    """-> [(outward normal, the four corners counter-clockwise seen from outside)]"""
    faces = []
    for axis in range(3):
        for side in (0, 1):
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            u = np.zeros(3)
            u[(axis + 1) % 3] = 1.0
            v = np.cross(n, u)                      # u x v = n
            on = [c for c in range(8) if CORNERS[c][axis] == side]
            centre = CORNERS[on].mean(0)
            on.sort(key=lambda c: np.arctan2((CORNERS[c] - centre) @ v, (CORNERS[c] - centre) @ u))
            faces.append((n, on))
    return faces


FACES = _faces()


def _directed(a, b, corner, n, corner_on_left):
    """the segment between edges a and b, directed so that `corner` lies on its left (or right) seen against n"""
    pa, pb = EDGE_MID[a], EDGE_MID[b]
    left = np.cross(pb - pa, CORNERS[corner] - pa) @ n > 0
    return (a, b) if left == corner_on_left else (b, a)


def case_segments(case, rule):
    segs = []
    for n, q in FACES:
        inside = [(case >> c) & 1 for c in q]
        edge = [EDGE_OF[frozenset((q[i], q[(i + 1) % 4]))] for i in range(4)]
        crossed = [i for i in range(4) if inside[i] != inside[(i + 1) % 4]]
        if len(crossed) == 2:
            c_in = q[inside.index(1)]
            segs.append(_directed(edge[crossed[0]], edge[crossed[1]], c_in, n, True))
        elif len(crossed) == 4:
            for i in range(4):
                if rule == "separate" and inside[i]:
                    segs.append(_directed(edge[(i - 1) % 4], edge[i], q[i], n, True))
                if rule == "join" and not inside[i]:
                    segs.append(_directed(edge[(i - 1) % 4], edge[i], q[i], n, False))
    return segs


def case_loops(case, rule=None):
    if case in EXCEPTIONS and rule is None:
        return [list(l) for l in EXCEPTIONS[case]]
    nxt = {}
    for a, b in case_segments(case, rule or FACE_RULE):
        assert a not in nxt, (case, "an edge starts two segments")
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), (case, "segments do not chain")
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def _in_one_face(edges):
    """do the cube edges `edges` all lie in one face of the cube"""
    pts = np.array([CORNERS[c] for e in edges for c in EDGE_ENDS[e]])
    return bool(((pts == 0).all(0) | (pts == 1).all(0)).any())


def _fan_start(loop):
    for start in sorted(loop):
        k = loop.index(start)
        rot = loop[k:] + loop[:k]
        if not any(_in_one_face((rot[0], rot[i], rot[i + 1])) for i in range(1, len(rot) - 1)):
            return rot
    raise AssertionError(("every fan of this loop holds a triangle inside a face", loop))


def case_triangles(case, rule=None, flip=None):
    flip = FLIP if flip is None else flip
    tris = []
    for loop in case_loops(case, rule):
        loop = _fan_start(loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i + 1], loop[i]) if flip else (loop[0], loop[i], loop[i + 1]))
    return tris


def tables(rule=None, flip=None):
    """-> edge_ends [12,2] int8, ntri [256] uint8, tri [256, 3*MAX_TRIS] int8 (-1 padded)"""
    ntri = np.zeros(256, np.uint8)
    tri = np.full((256, 3 * MAX_TRIS), -1, np.int8)
    for case in range(256):
        t = case_triangles(case, rule, flip)
        assert len(t) <= MAX_TRIS, (case, len(t))
        ntri[case] = len(t)
        tri[case, :3 * len(t)] = np.array(t, np.int8).reshape(-1)
    return np.array(EDGE_ENDS, np.int8), ntri, tri


def render():
    ends, ntri, tri = tables()
    out = ["// GENERATED by tools/gen_mcubes_tables.py -- do not edit; tests/test_mcubes_cpu.py regenerates and compares.",
           "// Corner c = 4*dx + 2*dy + dz; case bit c set when value[c] < isovalue; edges 0-3 along x, 4-7 along y, 8-11 along z.",
           f"// face rule: {FACE_RULE}; fan flipped: {int(FLIP)}; exceptions: {sorted(EXCEPTIONS)}",
           "#pragma once",
           "#include <stdint.h>",
           "",
           f"#define MCUBES_MAX_TRIS {MAX_TRIS}",
           "// corners an edge vertex is interpolated between: first + mu * (second - first)",
           "#define MCUBES_EDGE_ENDS_INIT { " + ", ".join("{%d, %d}" % (a, b) for a, b in ends) + " }",
           "// triangles a case emits",
           "#define MCUBES_NTRI_INIT { \\"]
    for r in range(0, 256, 32):
        out.append("    " + ", ".join(str(int(v)) for v in ntri[r:r + 32]) + ", \\")
    out[-1] = out[-1][:-3] + " }"
    out.append("// edge numbers of the triangles of a case, three per triangle, in emission order; -1 = unused")
    out.append("#define MCUBES_TRI_INIT { \\")
    for case in range(256):
        out.append("    { " + ", ".join("%2d" % int(v) for v in tri[case]) + " }, \\")
    out[-1] = out[-1][:-3] + " }"
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed header instead of writing")
    ap.add_argument("-o", default=HEADER)
    a = ap.parse_args()
    text = render()
    if a.check:
        same = open(a.o).read() == text
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(a.o, "w") as f:
        f.write(text)
    _, ntri, _ = tables()
    print(f"wrote {a.o}: {int(ntri.sum())} triangles over 256 cases, at most {int(ntri.max())}")


if __name__ == "__main__":
    main()
