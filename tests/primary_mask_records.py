"""Helper of the primary-mask tests: a scene's primitive records as the device reads them, restated in numpy."""
import numpy as np

import nori_hip as nh

PRIM_SPHERE = 1  # kPrimSphere: bit 0 of a record's last word (csrc/nh_layout.h)


def is_sphere(record) -> bool:
    return bool(int(np.asarray(record, np.float32)[11:12].view(np.int32)[0]) & PRIM_SPHERE)


def device_records(scene, bvh) -> np.ndarray:
    """(n, 12) float32 records in the order a context traverses them: record k is primitive bvh.indices()[k] (the
    reference's m_indices order, csrc/nh_traverse.h), primitive ids counted shape by shape (nh_bvh_desc.shape_offset).
    A triangle is (p0, 0) (p1, shape) (p2, 0), a sphere (centre, radius) (0, 0, 0, shape) (0, 0, 0, PRIM_SPHERE bits):
    the words the mask builder reads; the other flag bits of the device's records are left out."""
    d, b = scene.desc, bvh.desc
    V = np.ctypeslib.as_array(d.V, shape=(d.n_vertices, 3)) if d.n_vertices else np.zeros((0, 3), np.float32)
    F = np.ctypeslib.as_array(d.F, shape=(d.n_faces, 3)) if d.n_faces else np.zeros((0, 3), np.uint32)
    first = [int(b.shape_offset[i]) for i in range(b.n_shapes + 1)]
    recs = []
    for p in bvh.indices():
        i = int(np.searchsorted(first, int(p), side="right")) - 1
        s = d.shapes[i]
        r = np.zeros(12, np.float32)
        r[7] = i
        if s.type == nh.SHAPE_SPHERE:
            r[0:3], r[3] = s.center[:], s.radius
            r[11:12] = np.array([PRIM_SPHERE], np.int32).view(np.float32)
        else:
            f = F[s.f_offset + int(p) - first[i]]
            for j in range(3):
                r[4 * j:4 * j + 3] = V[s.v_offset + int(f[j])]
        recs.append(r)
    return np.array(recs, np.float32).reshape(-1, 12)
