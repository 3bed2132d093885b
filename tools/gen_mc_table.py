#!/usr/bin/env python3
"""Generates the marching-cubes case table of csrc/tsdf.hip (csrc/mc_table.h).

    python tools/gen_mc_table.py            # rewrites csrc/mc_table.h
    python tools/gen_mc_table.py --check    # fails when the committed header differs

Conventions.  Corner c of a cube sits at (c & 1, c >> 1 & 1, c >> 2 & 1); bit c
of a case is set when that corner is inside (tsdf < 0).  Edge e = 4 * axis + j
runs along `axis` from the corner whose two other coordinates are the bits of
j (x edges: j = y + 2 z, y edges: j = x + 2 z, z edges: j = x + 2 y).

Construction, per case.  On each of the six faces the crossed edges are joined
by segments: two crossings by one segment; four crossings (the two inside
corners diagonal) by two segments that each cut off one *inside* corner.  That
rule reads only the face's four signs, so the two cubes sharing a face draw the
same segments on it and the surface has no cracks.  Every segment is directed
so that the triangle it bounds has its normal on the outside (tsdf >= 0) side;
every crossed edge then ends exactly one segment and starts exactly one, the
segments chain into closed oriented loops, and each loop, started at its
lowest edge, is fan-triangulated from there.  Loops are listed by lowest edge.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd", "csrc", "mc_table.h")


def corner_pos(c):
    return (c & 1, c >> 1 & 1, c >> 2 & 1)


def edge_corners(e):
    """(corner a, corner b) of edge e, b = a + the axis bit."""
    axis, j = divmod(e, 4)
    others = [k for k in range(3) if k != axis]
    a = ((j & 1) << others[0]) | ((j >> 1) << others[1])
    return a, a | (1 << axis)


def edge_mid(e):
    a, b = edge_corners(e)
    pa, pb = corner_pos(a), corner_pos(b)
    return tuple((pa[k] + pb[k]) * 0.5 for k in range(3))


EDGE_OF = {edge_corners(e): e for e in range(12)}


def faces():
    """Per face: (outward normal, the four corners in cyclic order)."""
    out = []
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for side in (0, 1):
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                ring.append((side << axis) | (du << u) | (dv << v))
            out.append((tuple(n), ring))
    return out


FACES = faces()


def _sub(a, b):
    return tuple(a[k] - b[k] for k in range(3))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(a[k] * b[k] for k in range(3))


def _mean(ps):
    return tuple(sum(p[k] for p in ps) / len(ps) for k in range(3))


def _directed(ea, eb, away, normal):
    """The segment between the crossings of edges ea and eb, directed so that a triangle inside
    the cube with the segment on its boundary has its normal along `away` (the in-face direction
    from the inside corners to the outside ones)."""
    d = _sub(edge_mid(eb), edge_mid(ea))
    s = _dot(_cross(away, d), normal)
    assert abs(s) > 1e-9
    return (ea, eb) if s < 0 else (eb, ea)


def face_segments(case, normal, ring):
    inside = [bool(case >> c & 1) for c in ring]
    edges = []  # (position in the ring, edge id) of the crossed face edges
    for i in range(4):
        a, b = ring[i], ring[(i + 1) % 4]
        if inside[i] != inside[(i + 1) % 4]:
            edges.append((i, EDGE_OF[(min(a, b), max(a, b))]))
    if not edges:
        return []
    if len(edges) == 2:
        ins = _mean([corner_pos(c) for c, f in zip(ring, inside) if f])
        outs = _mean([corner_pos(c) for c, f in zip(ring, inside) if not f])
        return [_directed(edges[0][1], edges[1][1], _sub(outs, ins), normal)]
    assert len(edges) == 4
    segs = []
    for i in range(4):
        if not inside[i]:
            continue
        # ring edge i - 1 ends at corner i, ring edge i starts there
        ea = dict(edges)[(i - 1) % 4]
        eb = dict(edges)[i]
        mid = _mean([edge_mid(ea), edge_mid(eb)])
        segs.append(_directed(ea, eb, _sub(mid, corner_pos(ring[i])), normal))
    return segs


def case_triangles(case):
    """The triangles of one case as a flat list of edge ids, three per triangle."""
    crossed = [e for e in range(12) if (case >> edge_corners(e)[0] & 1) != (case >> edge_corners(e)[1] & 1)]
    segs = []
    for normal, ring in FACES:
        segs += face_segments(case, normal, ring)
    use = {e: 0 for e in crossed}
    nxt = {}
    for a, b in segs:
        use[a] += 1
        use[b] += 1
        assert a not in nxt, f"case {case}: edge {a} starts two segments"
        nxt[a] = b
    assert all(n == 2 for n in use.values()), f"case {case}: a crossed edge is not used by exactly two segments"
    assert sorted(nxt) == crossed and sorted(nxt.values()) == crossed
    tris, seen = [], set()
    for start in crossed:
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        for i in range(1, len(loop) - 1):
            tris += [loop[0], loop[i], loop[i + 1]]
    return tris


def build_table():
    rows = [case_triangles(c) for c in range(256)]
    width = max(len(r) for r in rows)
    return rows, width


def edge_mask(case):
    m = 0
    for e in range(12):
        a, b = edge_corners(e)
        if (case >> a & 1) != (case >> b & 1):
            m |= 1 << e
    return m


def render():
    rows, width = build_table()
    out = ["// mc_table.h — generated by tools/gen_mc_table.py; do not edit.",
           "// Corner c at (c & 1, c >> 1 & 1, c >> 2 & 1), case bit c set when the corner is inside;",
           "// edge e = 4 * axis + j (x: j = y + 2 z, y: j = x + 2 z, z: j = x + 2 y).",
           "#pragma once",
           "#include <stdint.h>",
           "",
           "#ifndef GSR_MC_TABLE_ATTR  // device code defines it as __constant__ const",
           "#define GSR_MC_TABLE_ATTR static const",
           "#endif",
           "",
           f"#define GSR_MC_ROW {width}  // the widest row: {width // 3} triangles",
           "",
           "// triangles per case",
           "GSR_MC_TABLE_ATTR uint8_t kMcNumTris[256] = {"]
    for i in range(0, 256, 32):
        out.append("    " + ", ".join(str(len(r) // 3) for r in rows[i:i + 32]) + ",")
    out += ["};", "", "// the crossed edges of a case, bit e", "GSR_MC_TABLE_ATTR uint16_t kMcEdgeMask[256] = {"]
    for i in range(0, 256, 16):
        out.append("    " + ", ".join(f"0x{edge_mask(c):03x}" for c in range(i, i + 16)) + ",")
    out += ["};", "", "// three edge ids per triangle, -1 past the end", "GSR_MC_TABLE_ATTR int8_t kMcTris[256][GSR_MC_ROW] = {"]
    for r in rows:
        out.append("    {" + ", ".join(f"{v:2d}" for v in r + [-1] * (width - len(r))) + "},")
    out += ["};", ""]
    return "\n".join(out)


def main(argv):
    text = render()
    _, width = build_table()
    if "--check" in argv:
        with open(HEADER) as fh:
            if fh.read() != text:
                print("mc_table.h differs from the generator's output", file=sys.stderr)
                return 1
        print(f"mc_table.h is current (widest row: {width // 3} triangles)")
        return 0
    with open(HEADER, "w") as fh:
        fh.write(text)
    print(f"wrote {HEADER} (widest row: {width // 3} triangles)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
