"""Writes the small mesh files of the reference cases (tests/data/ref_cases/*.obj, and the binary tests/golden/ref_inputs/*.ply).  Inputs of our own; run once and
commit the output.  Every file is a few KB: an icosphere (80 faces) with and without normals as OBJ and as binary PLY, a
cube of quads, and the tie / degenerate geometry of ties.xml."""
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# binary files live under tests/golden/ (the XMLs name them by relative path)
BINARY = os.path.normpath(os.path.join(HERE, "..", "..", "golden", "ref_inputs"))


def icosphere():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    mid = {}
    out = []
    for a, b, c in F:
        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = V[i] + V[j]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.array(V, dtype=np.float32), np.array(out, dtype=np.int32)


def write_obj(name, V, F, N=None, quads=None, head=""):
    with open(os.path.join(HERE, name), "w") as f:
        f.write("# " + head + "\n")
        for v in V:
            f.write("v %.9g %.9g %.9g\n" % tuple(v))
        if N is not None:
            for n in N:
                f.write("vn %.9g %.9g %.9g\n" % tuple(n))
        for t in ([] if F is None else F):
            f.write("f " + " ".join(("%d//%d" % (i + 1, i + 1)) if N is not None else str(i + 1) for i in t) + "\n")
        for q in ([] if quads is None else quads):
            f.write("f " + " ".join(str(i + 1) for i in q) + "\n")


def write_ply(name, V, F, N=None, index_type="int"):
    h = ["ply", "format binary_little_endian 1.0", "comment icosphere, 80 faces", "element vertex %d" % len(V),
         "property float x", "property float y", "property float z"]
    if N is not None:
        h += ["property float nx", "property float ny", "property float nz"]
    h += ["element face %d" % len(F), "property list uchar %s vertex_indices" % index_type, "end_header"]
    b = ("\n".join(h) + "\n").encode()
    for k, v in enumerate(V):
        b += struct.pack("<3f", *v)
        if N is not None:
            b += struct.pack("<3f", *N[k])
    code = {"int": "i", "ushort": "H"}[index_type]
    for t in F:
        b += struct.pack("<B3" + code, 3, *[int(i) for i in t])
    os.makedirs(BINARY, exist_ok=True)
    with open(os.path.join(BINARY, name), "wb") as f:
        f.write(b)


if __name__ == "__main__":
    V, F = icosphere()
    write_obj("ico.obj", V, F, head="icosphere, 42 vertices, 80 faces, NO normals: the parser computes them")
    # normals that are NOT the positions, so that a pipeline which recomputed them would show: tilted towards +y
    N = V + np.array([0, 0.35, 0], dtype=np.float32)
    write_obj("ico_normals.obj", V, F, N=N, head="the same icosphere with explicit (unnormalised, tilted) normals")
    write_ply("ico.ply", V, F)
    write_ply("ico_normals.ply", V, F, N=(N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32), index_type="ushort")
    C = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    Q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    write_obj("cube_quads.obj", C, None, quads=Q, head="axis-aligned cube of six QUADS sharing all their edges, no normals")
    # ties.obj: a unit quad in the plane z = 0 as two triangles, THE SAME two triangles again (coincident duplicates, other
    # vertices so that they are not merged), a second quad sharing the edge x = 1, and one zero-area triangle
    T = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0),
                  (0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0),
                  (2, 0, 0), (2, 1, 0),
                  (0.25, 0.25, 0.5), (0.5, 0.5, 0.5), (0.75, 0.75, 0.5)], dtype=np.float32)
    TF = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (1, 8, 9), (1, 9, 2), (10, 11, 12)]
    TN = np.tile(np.array([0, 0, 1], dtype=np.float32), (len(T), 1))
    TN[4:8] = (0, 0.6, 0.8)      # the duplicates carry another normal: the recorded shading normal tells which twin won the tie
    write_obj("ties.obj", T, TF, N=TN, head="coincident duplicate triangles, quads sharing an edge, one zero-area triangle")
