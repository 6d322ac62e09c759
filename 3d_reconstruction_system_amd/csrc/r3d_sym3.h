// The symmetric 3x3 eigenproblem in fp64, stated once for the device (r3d_knn.hip: the normals' covariance, one per lane) and
// the host (r3d_ransac.hip: the refit's covariance, one per call): cyclic Jacobi sweeps over scalars, nothing indexed at run
// time.  The library is built -ffp-contract=off, so both sides run the same sequence of IEEE operations: the same bits.
#pragma once

#include <cmath>

#include "r3d_sums_dev.h"   // R3D_HD

namespace r3d_sym3 {

// One Jacobi rotation of the symmetric 3x3 (diagonal app, aqq; off-diagonal apq; arp, arq the third row's entries) and of the
// eigenvector columns p, q; returns false when apq is already negligible next to the diagonal (2^-64 of it).
R3D_HD __forceinline__ bool jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                          double& v1p, double& v1q, double& v2p, double& v2q) {
  if (!(fabs(apq) > 5.421010862427522e-20 * (fabs(app) + fabs(aqq)))) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double at = fabs(theta);
  double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
  t = theta < 0.0 ? -t : t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = rp - s * (rq + tau * rp);
  arq = rq + s * (rp - tau * rq);
  double p, q;
  p = v0p, q = v0q, v0p = p - s * (q + tau * p), v0q = q + s * (p - tau * q);
  p = v1p, q = v1q, v1p = p - s * (q + tau * p), v1q = q + s * (p - tau * q);
  p = v2p, q = v2q, v2p = p - s * (q + tau * p), v2q = q + s * (p - tau * q);
  return true;
}

// Eigenvalues l[0] <= l[1] <= l[2] of the symmetric C (xx, xy, xz, yy, yz, zz) and the unit eigenvector of l[0] (the lowest
// column on ties).
R3D_HD __forceinline__ void sym3_smallest(const double C[6], double l[3], double n[3]) {
  double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool any = jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    any |= jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    any |= jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    if (!any) break;
  }
  const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
  l[0] = fmin(a00, fmin(a11, a22));
  l[2] = fmax(a00, fmax(a11, a22));
  l[1] = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
  const double x = c0 ? v00 : c1 ? v01 : v02, y = c0 ? v10 : c1 ? v11 : v12, z = c0 ? v20 : c1 ? v21 : v22;
  const double len = sqrt(x * x + y * y + z * z);
  n[0] = x / len;
  n[1] = y / len;
  n[2] = z / len;
}

}  // namespace r3d_sym3
