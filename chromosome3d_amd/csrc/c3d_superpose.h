// c3d_superpose.h — the per-pair arithmetic of the superposition kernels (c3d_score_superpose.inc k_sup_solve), free of the HIP runtime so that the
// same lines compile for the host: the least-squares rotation of one centred model onto another from their 3 x 3 covariance.
//
// Horn (J. Opt. Soc. Am. A 4, 629, 1987): with S = sum a_i b_i^T, the unit quaternion of the rotation R that minimises sum |R a_i - b_i|^2
// is the eigenvector of the largest eigenvalue lambda of the symmetric 4 x 4 matrix N(S) below, and the minimum is G_a + G_b - 2 lambda.
// An improper fit of a (a rotation after the reflection a -> -a through the origin) is a proper fit of -a, whose matrix is N(-S) = -N(S):
// cyclic Jacobi on -N makes the rotations it makes on N (every angle is a ratio of two entries), so one diagonalisation serves both
// candidates — the proper fit owns the largest eigenpair of N, the reflected fit the smallest with its eigenvalue negated.
// The eigenpairs come from kSupSweeps cyclic sweeps of six Jacobi rotations each, a fixed count: a 4 x 4 symmetric matrix is diagonal to
// fp64 rounding after five or six (the off-diagonal norm falls quadratically), ten leave a margin.  Nothing here loops on data.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define C3D_HD __host__ __device__ __forceinline__
#else
#define C3D_HD inline
#endif

namespace c3d {

constexpr int kSupSweeps = 10;
constexpr int kSupCov = 11;      // sums a pair holds: S row-major (S[3 r + c] = sum a_r b_c), then G_a = sum |a|^2 and G_b = sum |b|^2
constexpr int kSupFit = 12;      // a pair's fit: Q row-major (9), mirrored (0 / 1 as a double), the winning eigenvalue, 0

// one Jacobi rotation in the (P, Q) plane of the symmetric A (full storage), accumulated into the columns of V
template <int P, int Q>
C3D_HD void sup_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    double c = 1.0, s = 0.0;
    if (apq != 0.0) {
        const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        c = 1.0 / sqrt(t * t + 1.0);
        s = t * c;
    }
    for (int k = 0; k < 4; ++k) {          // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
    for (int k = 0; k < 4; ++k) {          // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// cov: kSupCov sums of the pair (a, b).  allow_mirror: the reflected candidate takes part.  fit: kSupFit doubles — Q with Q a ~ b
// (orthogonal, det +1, or det -1 when mirrored: the reflection is folded in), the mirror bit, the eigenvalue of the chosen candidate.
C3D_HD void sup_solve(const double* cov, bool allow_mirror, double* fit) {
    const double Sxx = cov[0], Sxy = cov[1], Sxz = cov[2], Syx = cov[3], Syy = cov[4], Syz = cov[5], Szx = cov[6], Szy = cov[7], Szz = cov[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < kSupSweeps; ++sweep) {
        sup_rotate<0, 1>(A, V); sup_rotate<0, 2>(A, V); sup_rotate<0, 3>(A, V);
        sup_rotate<1, 2>(A, V); sup_rotate<1, 3>(A, V); sup_rotate<2, 3>(A, V);
    }
    // the largest and the smallest eigenvalue and their vectors, by selection (no indexed register)
    double lmax = A[0][0], lmin = A[0][0];
    double qmax[4] = {V[0][0], V[1][0], V[2][0], V[3][0]}, qmin[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
    for (int k = 1; k < 4; ++k) {
        const bool up = A[k][k] > lmax, down = A[k][k] < lmin;
        lmax = up ? A[k][k] : lmax;
        lmin = down ? A[k][k] : lmin;
        for (int r = 0; r < 4; ++r) {
            qmax[r] = up ? V[r][k] : qmax[r];
            qmin[r] = down ? V[r][k] : qmin[r];
        }
    }
    const bool mir = allow_mirror && -lmin > lmax;
    const double sg = mir ? -1.0 : 1.0;
    double q0 = mir ? qmin[0] : qmax[0], q1 = mir ? qmin[1] : qmax[1], q2 = mir ? qmin[2] : qmax[2], q3 = mir ? qmin[3] : qmax[3];
    const double inv = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    q0 *= inv; q1 *= inv; q2 *= inv; q3 *= inv;
    fit[0] = sg * (q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3);
    fit[1] = sg * (2.0 * (q1 * q2 - q0 * q3));
    fit[2] = sg * (2.0 * (q1 * q3 + q0 * q2));
    fit[3] = sg * (2.0 * (q1 * q2 + q0 * q3));
    fit[4] = sg * (q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3);
    fit[5] = sg * (2.0 * (q2 * q3 - q0 * q1));
    fit[6] = sg * (2.0 * (q1 * q3 - q0 * q2));
    fit[7] = sg * (2.0 * (q2 * q3 + q0 * q1));
    fit[8] = sg * (q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3);
    fit[9] = mir ? 1.0 : 0.0;
    fit[10] = mir ? -lmin : lmax;
    fit[11] = 0.0;
}

// the identity fit: a model onto itself (the diagonal of the table, the reference replica)
C3D_HD void sup_identity(double* fit) {
    for (int k = 0; k < kSupFit; ++k) fit[k] = 0.0;
    fit[0] = fit[4] = fit[8] = 1.0;
}

}  // namespace c3d
