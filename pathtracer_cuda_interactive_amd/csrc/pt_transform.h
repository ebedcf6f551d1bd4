// pt_transform.h — the rule of pt_scene_transform (include/pt_api.h), written once for the device kernel of
// pt_scene_transform.hip, for the host half's preparation of the group table and for the host twins
// pt_transform_geometry_host / pt_transform_sphere_host: a row-major 3x4 matrix applied to the points, vertex normals and
// spheres of a primitive record.
//
// Every operation is an IEEE fp32 + - * in the order written (no contraction: the build forbids it) and one correctly rounded
// square root, so the device, the host twin and a numpy restatement give the same bits.
//
// Layout: one 84-B entry per group, the 12 matrix entries as the caller gave them, then the 9 entries of the normal matrix
// (the cofactors of the linear part, negated where its determinant is negative), made once per group on the host.
#pragma once

#include <stdint.h>

#include <initializer_list>
#include <string>

#include "../../include/pt_api.h"
#include "pt_math.h"

namespace ptx {

struct Entry { float m[12]; float c[9]; };
static_assert(sizeof(Entry) == 84, "Entry must be 84 bytes");
constexpr int kEntryFloats = 21;

PT_HD bool finite32(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }   // false for inf and NaN

// x' = ((m0 x + m1 y) + m2 z) + m3, rows 1 and 2 alike
PT_HD ptm::V3 point(const float* m, ptm::V3 p) {
    return ptm::mk(((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3],
                   ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7],
                   ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]);
}

// n'.x = (c0.x nx + c0.y ny) + c0.z nz, the other components alike; not renormalised (make_surface normalises after interpolation)
PT_HD ptm::V3 normal(const float* c, ptm::V3 n) {
    return ptm::mk((c[0] * n.x + c[1] * n.y) + c[2] * n.z,
                   (c[3] * n.x + c[4] * n.y) + c[5] * n.z,
                   (c[6] * n.x + c[7] * n.y) + c[8] * n.z);
}

// r' = r * sqrt((m0 m0 + m4 m4) + m8 m8): the length of the linear part's first column (a similarity scales every direction alike)
PT_HD float radius(const float* m, float r) { return r * ptm::sqrt_exact((m[0] * m[0] + m[4] * m[4]) + m[8] * m[8]); }

// The group entry of a matrix.  0, or — with *e untouched — 1 + i where m[i] is not finite, 13 where the determinant is 0 or NaN
// (both: an argument the rule refuses), 14 where a cofactor overflowed (a result that is not finite: every normal would be).
inline int prepare(const pt_transform* t, Entry* e) {
    const float* m = t->m;
    for (int k = 0; k < 12; k++)
        if (!finite32(m[k])) return 1 + k;
    const ptm::V3 r0 = ptm::mk(m[0], m[1], m[2]), r1 = ptm::mk(m[4], m[5], m[6]), r2 = ptm::mk(m[8], m[9], m[10]);
    ptm::V3 c0 = ptm::cross(r1, r2), c1 = ptm::cross(r2, r0), c2 = ptm::cross(r0, r1);
    const float det = ptm::dot(r0, c0);
    if (!(det != 0.0f)) return 13;                        // 0 or NaN
    if (det < 0.0f) { c0 = -c0; c1 = -c1; c2 = -c2; }
    for (float v : {c0.x, c0.y, c0.z, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z})
        if (!finite32(v)) return 14;
    for (int k = 0; k < 12; k++) e->m[k] = m[k];
    e->c[0] = c0.x; e->c[1] = c0.y; e->c[2] = c0.z;
    e->c[3] = c1.x; e->c[4] = c1.y; e->c[5] = c1.z;
    e->c[6] = c2.x; e->c[7] = c2.y; e->c[8] = c2.z;
    return 0;
}

// what a refusal of prepare says
inline std::string refusal(int code) {
    return code == 14 ? std::string("its normal matrix (the cofactors of the linear part) is not finite")
         : code == 13 ? std::string("the determinant of its linear part is 0 or NaN (singular)")
                      : "m[" + std::to_string(code - 1) + "] is not finite";
}
inline int refusal_status(int code) { return code == 14 ? PT_ERR_UNSUPPORTED : PT_ERR_INVALID_ARG; }

}  // namespace ptx
