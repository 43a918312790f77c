// Geometry shared by the two-view solvers (k_relpose.hip: five-point essential matrix; k_fundamental.hip: 7-point / 8-point fundamental
// matrix).  Host-compilable: tests/test_relpose_emulated.py and tests/test_fundamental_emulated.py put the text between the two markers
// below in front of a solver's own slice, drop the __device__ qualifiers and compile both with the host compiler, so nothing in this
// file may need the device (no LDS declarations, no inline machine code, no target builtins: the tests check the whole file for them).
// Only + - * / and comparisons, every product and sum rounded once: the numpy restatements repeat these operations in this order.
#pragma once

#pragma clang fp contract(off)

namespace xfh {
// ---- twoview math begin ----
namespace tv {
constexpr double PIVOT_EPS = 1e-12;          // gauss_jordan: a pivot below it (or not finite) is a degenerate system

// per-thread working set in LDS: element k of thread j at b[k * ST + j] (consecutive lanes, consecutive banks); ST = 1 on the host
template <int ST>
struct Slice {
    double* b;
    __device__ inline double& operator[](int k) const { return b[k * ST]; }
};

__device__ inline bool is_finite(double v) { return v - v == 0.0; }
__device__ inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// orthonormal frame (e1, e2, e3) of the triangle (A, B, C): e1 = (B - A) / |.|, e3 = (e1 x (C - A)) / |.|, e2 = e3 x e1; false: degenerate
// (a zero first side, or sin^2 of the angle at A <= collinear_eps2).  Shared by k_abspose.hip (ap_frame) and k_align.hip (al_solve).
__device__ inline bool triangle_frame(const double* A, const double* B, const double* Cc, double collinear_eps2, double* e1, double* e2, double* e3) {
    const double d1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const double d2[3] = {Cc[0] - A[0], Cc[1] - A[1], Cc[2] - A[2]};
    const double n1 = dot3(d1, d1);
    const double r1 = sqrt(n1);
#pragma unroll
    for (int k = 0; k < 3; ++k) e1[k] = d1[k] / r1;
    double c[3];
    cross3(e1, d2, c);
    const double n3 = dot3(c, c), n2 = dot3(d2, d2);
    const double r3 = sqrt(n3);
#pragma unroll
    for (int k = 0; k < 3; ++k) e3[k] = c[k] / r3;
    cross3(e3, e1, e2);
    return n1 > 0.0 && n3 > collinear_eps2 * n2;
}

// Sampson error of x0 = (a, b, 1), x1 = (c, d, 1) under M = E or F (x1' M x0 = 0)
__device__ inline double sampson(const double* M, double a, double b, double c, double d) {
    const double e0 = (M[0] * a + M[1] * b) + M[2], e1 = (M[3] * a + M[4] * b) + M[5], e2 = (M[6] * a + M[7] * b) + M[8];
    const double f0 = (M[0] * c + M[3] * d) + M[6], f1 = (M[1] * c + M[4] * d) + M[7];
    const double num = (c * e0 + d * e1) + e2;
    const double den = ((e0 * e0 + e1 * e1) + f0 * f0) + f1 * f1;
    return num * num / den;
}

// Gauss-Jordan with partial pivoting on the first `rows` columns of a rows x cols matrix at S[base + r * cols + c]; false if degenerate
template <class S>
__device__ inline bool gauss_jordan(S s, int base, int rows, int cols) {
    for (int c = 0; c < rows; ++c) {
        int p = c;
        double best = fabs(s[base + c * cols + c]);
        for (int r = c + 1; r < rows; ++r) {
            const double v = fabs(s[base + r * cols + c]);
            if (v > best) { best = v; p = r; }
        }
        if (!(best >= PIVOT_EPS)) return false;
        if (p != c)
            for (int j = c; j < cols; ++j) {
                const double tmp = s[base + c * cols + j];
                s[base + c * cols + j] = s[base + p * cols + j];
                s[base + p * cols + j] = tmp;
            }
        const double inv = 1.0 / s[base + c * cols + c];
        for (int j = c + 1; j < cols; ++j) s[base + c * cols + j] = s[base + c * cols + j] * inv;
        s[base + c * cols + c] = 1.0;
        for (int r = 0; r < rows; ++r) {
            if (r == c) continue;
            const double f = s[base + r * cols + c];
            for (int j = c + 1; j < cols; ++j) s[base + r * cols + j] = s[base + r * cols + j] - f * s[base + c * cols + j];
            s[base + r * cols + c] = 0.0;
        }
    }
    return true;
}

// poly product c[0..da+db] = a * b (ascending powers), accumulated in the order i, j
__device__ inline void pmul(const double* a, int da, const double* b, int db, double* c) {
    for (int k = 0; k <= da + db; ++k) c[k] = 0.0;
    for (int i = 0; i <= da; ++i)
        for (int j = 0; j <= db; ++j) c[i + j] = c[i + j] + a[i] * b[j];
}
}  // namespace tv
// ---- twoview math end ----
}  // namespace xfh
