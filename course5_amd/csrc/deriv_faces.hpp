// What the geometry derivatives share: the two faces of a cell a pixel's ray runs between, how a face's depth moves with an
// affine field or with its three vertices, the chord terms, and the view's rotation chain.
#pragma once

#include "deriv_ray.hpp"

namespace c5 {
namespace adj {

// vertex k (face_plane's order) of face f of a cell, as an index into the cell's four
__device__ __forceinline__ constexpr int face_vertex(int f, int k) {
    constexpr int FV[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    return FV[f][k];
}

// the three points of face f of the cell cv, in face_plane's order (face_vertex on the cell's point ids)
__device__ __forceinline__ void face_points(int4 cv, int f, int (&v)[3]) {
    v[0] = f == 3 ? cv.y : cv.x;
    v[1] = f <= 1 ? cv.y : cv.z;
    v[2] = f == 0 ? cv.z : cv.w;
}

__device__ __forceinline__ void load_vertices(const MotionGeometry& G, int4 cv, double (&p)[4][3]) {
    const int vid[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k][0] = G.vx[vid[k]];
        p[k][1] = G.vy[vid[k]];
        p[k][2] = G.vz[vid[k]];
    }
}

// The two faces of a cell the ray of pixel (x, y) runs between, from the cell's view-space vertices p: a tetrahedron is
// convex, so among the faces it lies ABOVE (face_plane: kind < 0; a ray along +z enters through one of them) the one met
// is the deepest at (x, y), and among those it lies below the shallowest.  Faces edge-on to rounding (kind 0) are never
// candidates.  found: both exist.  The rule is written three times, once per result a walk kernel wants - cell_faces (the
// vertex tangent: index, barycentric coordinates l0, l1, l2 for the face's vertices in face_plane's order, slopes),
// cell_faces_bary (the vertex adjoint: without the slopes) and cell_slopes (the motion tangent: depth and slopes).  As
// views of one function the walk kernels compile to other code, and motion_walk<8> and vertex_walk<true> ran 1 % slower
// (profiles/experiments.md).  The vertex tangent is the transpose of the vertex adjoint only while the first two agree.
struct FaceBary {
    int f;
    double l0, l1, l2;
};
struct CellFacesBary {
    FaceBary in, out;
    bool found;
};
struct CellFaces {
    CellFacesBary b;
    double gx_in, gy_in, gx_out, gy_out;
};
__device__ __forceinline__ CellFaces cell_faces(const double (&p)[4][3], double x, double y) {
    double w_in = -INFINITY, w_out = INFINITY;
    double in_n1 = 0.0, in_n2 = 0.0, in_m = 1.0, out_n1 = 0.0, out_n2 = 0.0, out_m = 1.0;
    CellFaces r;
    r.gx_in = r.gy_in = r.gx_out = r.gy_out = 0.0;
    int f_in = 0, f_out = 0;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        const double w = fma(fp.gx, x - p[0][0], fma(fp.gy, y - p[0][1], fp.c));
        const double* a = p[face_vertex(f, 0)];
        const double* b = p[face_vertex(f, 1)];
        const double* c = p[face_vertex(f, 2)];
        const double m = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]);
        const double n1 = (x - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (y - a[1]);
        const double n2 = (b[0] - a[0]) * (y - a[1]) - (x - a[0]) * (b[1] - a[1]);
        if (fp.kind < 0 && w > w_in) {
            w_in = w;
            f_in = f;
            in_n1 = n1, in_n2 = n2, in_m = m;
            r.gx_in = fp.gx, r.gy_in = fp.gy;
        }
        if (fp.kind > 0 && w < w_out) {
            w_out = w;
            f_out = f;
            out_n1 = n1, out_n2 = n2, out_m = m;
            r.gx_out = fp.gx, r.gy_out = fp.gy;
        }
    }
    r.b.found = w_in > -INFINITY && w_out < INFINITY;
    r.b.in.f = f_in;
    r.b.in.l1 = in_n1 / in_m;
    r.b.in.l2 = in_n2 / in_m;
    r.b.in.l0 = 1.0 - r.b.in.l1 - r.b.in.l2;
    r.b.out.f = f_out;
    r.b.out.l1 = out_n1 / out_m;
    r.b.out.l2 = out_n2 / out_m;
    r.b.out.l0 = 1.0 - r.b.out.l1 - r.b.out.l2;
    return r;
}

// the vertex adjoint's form
__device__ __forceinline__ CellFacesBary cell_faces_bary(const double (&p)[4][3], double x, double y) {
    double w_in = -INFINITY, w_out = INFINITY;
    // of the face chosen so far: the numerators of l1 and l2 and their denominator (divided once, behind the loop)
    double in_n1 = 0.0, in_n2 = 0.0, in_m = 1.0, out_n1 = 0.0, out_n2 = 0.0, out_m = 1.0;
    int f_in = 0, f_out = 0;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        const double w = fma(fp.gx, x - p[0][0], fma(fp.gy, y - p[0][1], fp.c));
        const double* a = p[face_vertex(f, 0)];
        const double* b = p[face_vertex(f, 1)];
        const double* c = p[face_vertex(f, 2)];
        const double m = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]);
        const double n1 = (x - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (y - a[1]);
        const double n2 = (b[0] - a[0]) * (y - a[1]) - (x - a[0]) * (b[1] - a[1]);
        if (fp.kind < 0 && w > w_in) {
            w_in = w;
            f_in = f;
            in_n1 = n1, in_n2 = n2, in_m = m;
        }
        if (fp.kind > 0 && w < w_out) {
            w_out = w;
            f_out = f;
            out_n1 = n1, out_n2 = n2, out_m = m;
        }
    }
    CellFacesBary r;
    r.found = w_in > -INFINITY && w_out < INFINITY;
    r.in.f = f_in;
    r.in.l1 = in_n1 / in_m;
    r.in.l2 = in_n2 / in_m;
    r.in.l0 = 1.0 - r.in.l1 - r.in.l2;
    r.out.f = f_out;
    r.out.l1 = out_n1 / out_m;
    r.out.l2 = out_n2 / out_m;
    r.out.l0 = 1.0 - r.out.l1 - r.out.l2;
    return r;
}
// the motion tangent's form, for `cell` by its id
struct FaceAt {
    double w, gx, gy;
};
struct CellSlopes {
    FaceAt in, out;
    bool found;
};
__device__ __forceinline__ CellSlopes cell_slopes(const MotionGeometry& G, int cell, double x, double y) {
    double p[4][3];
    load_vertices(G, G.cell_vert[cell], p);
    CellSlopes r;
    r.in = FaceAt{-INFINITY, 0.0, 0.0};
    r.out = FaceAt{INFINITY, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        const double w = fma(fp.gx, x - p[0][0], fma(fp.gy, y - p[0][1], fp.c));
        if (fp.kind < 0 && w > r.in.w) r.in = FaceAt{w, fp.gx, fp.gy};
        if (fp.kind > 0 && w < r.out.w) r.out = FaceAt{w, fp.gx, fp.gy};
    }
    r.found = r.in.w > -INFINITY && r.out.w < INFINITY;
    return r;
}

// dw = u_z(P) - gx u_x(P) - gy u_y(P) at P = (x, y, w) for the field f = {A row-major, b}: how the depth of a face of
// slopes (gx, gy) moves at the pixel.  w is the innermost term: nothing of this is invariant along the ray, so the
// compiler keeps no per-field registers for it.
__device__ __forceinline__ double face_dw(const double* f, double gx, double gy, double x, double y, double w) {
    const double ux = fma(f[0], x, fma(f[1], y, fma(f[2], w, f[9])));
    const double uy = fma(f[3], x, fma(f[4], y, fma(f[5], w, f[10])));
    const double uz = fma(f[6], x, fma(f[7], y, fma(f[8], w, f[11])));
    return fma(-gy, uy, fma(-gx, ux, uz));
}

// lambda (u_z - gx u_x - gy u_y) of one vertex: u = its three doubles of one field
__device__ __forceinline__ double vertex_dw(const double* __restrict__ u, double l, double gx, double gy) {
    return l * fma(-gy, u[1], fma(-gx, u[0], u[2]));
}

// ddz = dw_exit - dw_entry of one field: six gathers of three doubles.  u: the field's first double of point 0, pitch
// doubles from point to point.  This is ALL of a field's arithmetic that touches the velocities: the same at every width.
__device__ __forceinline__ double vertex_ddz(const double* __restrict__ u, size_t pitch, const int (&vo)[3], const int (&vi)[3],
                                             const CellFaces& cf) {
    const double dw_out = vertex_dw(u + vo[0] * pitch, cf.b.out.l0, cf.gx_out, cf.gy_out) +
                          vertex_dw(u + vo[1] * pitch, cf.b.out.l1, cf.gx_out, cf.gy_out) +
                          vertex_dw(u + vo[2] * pitch, cf.b.out.l2, cf.gx_out, cf.gy_out);
    const double dw_in = vertex_dw(u + vi[0] * pitch, cf.b.in.l0, cf.gx_in, cf.gy_in) +
                         vertex_dw(u + vi[1] * pitch, cf.b.in.l1, cf.gx_in, cf.gy_in) +
                         vertex_dw(u + vi[2] * pitch, cf.b.in.l2, cf.gx_in, cf.gy_in);
    return dw_out - dw_in;
}

// d I_k / d dz_k of an active segment (the clamp is on alpha, not on the chord)
__device__ __forceinline__ double chord_dI(double a, double q, double E, double I_prev) { return E * fma(-a, I_prev, q); }

// One rotation of the view's linear part, mixing u (y for axis 0, x for axis 1) with z: u' = c u - s z, z' = s u + c z;
// TRANSPOSED: u' = c u + s z, z' = c z - s u.  Each direction keeps the expressions its kernel had: how the compiler
// contracts them is part of the result's last bits.
template <bool TRANSPOSED>
__device__ __forceinline__ void rotate_pair(double c, double s, double& u, double& z) {
    const double t = u;
    u = TRANSPOSED ? c * t + s * z : c * t - s * z;
    z = TRANSPOSED ? c * z - s * t : s * t + c * z;
}
// The linear part M of the view applied to (x, y, z): its rotations in order (their centres drop out of the linear part).
// TRANSPOSED: M^T, the rotations transposed in reverse order.
template <bool TRANSPOSED>
__device__ __forceinline__ void rotate_linear(const RotationList& R, double& x, double& y, double& z) {
    for (int k = 0; k < R.n; ++k) {
        const int r = TRANSPOSED ? R.n - 1 - k : k;
        if (R.axis[r] == 0) rotate_pair<TRANSPOSED>(R.cosv[r], R.sinv[r], y, z);
        else rotate_pair<TRANSPOSED>(R.cosv[r], R.sinv[r], x, z);
    }
}

}  // namespace adj
}  // namespace c5
