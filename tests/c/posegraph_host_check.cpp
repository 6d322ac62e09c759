// Stand-alone host program over csrc/r3d_posegraph.cpp for AddressSanitizer / UndefinedBehaviorSanitizer (no GPU, no Python):
// a ring of 12 poses with one wrong uncertain chord, with and without robust weights, a single node, a refused graph and the
// information matrix.  Returns non-zero when an answer is off.  tests/test_posegraph_host.py builds it with
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -I<csrc> -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=undefined -x hip <csrc>/r3d_posegraph.cpp tests/c/posegraph_host_check.cpp
//         -fsanitize=address,undefined
// and runs it.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "r3d.h"
void r3d_set_error(const char* fmt, ...) { (void)fmt; }
static void pose(double* T, double yaw, double x, double y, double z) {
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double M[16] = {c, 0, s, x, 0, 1, 0, y, -s, 0, c, z, 0, 0, 0, 1};
  for (int k = 0; k < 16; ++k) T[k] = M[k];
}
static void mul(const double* A, const double* B, double* C) {
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { double v = 0; for (int k = 0; k < 4; ++k) v += A[4*r+k]*B[4*k+c]; C[4*r+c] = v; }
}
static void inv(const double* A, double* B) {
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) B[4*r+c] = A[4*c+r]; B[4*r+3] = -(A[r]*A[3] + A[4+r]*A[7] + A[8+r]*A[11]); }
  B[12] = B[13] = B[14] = 0; B[15] = 1;
}
int main() {
  int bad = 0;
  const int n = 12;
  std::vector<double> truth(16 * n), start(16 * n);
  for (int i = 0; i < n; ++i) { pose(&truth[16*i], 0.3 * i, i, 0.1 * i, -0.2 * i); pose(&start[16*i], 0.3 * i + (i ? 0.05 : 0), i + (i ? 0.03 : 0), 0.1 * i, -0.2 * i); }
  std::vector<int32_t> nodes; std::vector<double> Ts, Ls; std::vector<uint8_t> unc;
  auto edge = [&](int s, int t, bool u, bool wrong) {
    double it[16], T[16]; inv(&truth[16*t], it); mul(it, &truth[16*s], T);
    if (wrong) { T[3] += 3.0; }
    nodes.push_back(s); nodes.push_back(t); for (int k = 0; k < 16; ++k) Ts.push_back(T[k]);
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) Ls.push_back(r == c ? 1000.0 : 0.0);
    unc.push_back(u);
  };
  for (int i = 0; i < n; ++i) edge((i + 1) % n, i, false, false);
  edge(5, 0, true, false); edge(9, 2, true, true); edge(11, 4, true, false);
  std::vector<double> w(unc.size()), rep(8);
  for (double pref : {1.0, (double)INFINITY}) {
    std::vector<double> p = start;
    int rc = r3d_posegraph_optimize(n, p.data(), (int)unc.size(), nodes.data(), Ts.data(), Ls.data(), unc.data(), 0.05, pref, 0.25, 100, w.data(), rep.data());
    double worst = 0; for (size_t k = 0; k < p.size(); ++k) worst = std::fmax(worst, std::fabs(p[k] - truth[k]));
    bad += rc != 0 || (pref == 1.0 ? !(worst < 1e-9 && rep[3] == 1) : !(worst > 0.1 && rep[3] == 0));
    std::printf("pref %g rc %d cost %.3g -> %.3g iters %g pruned %g status %g worst %.3g\n", pref, rc, rep[0], rep[1], rep[2], rep[3], rep[4], worst);
  }
  double one[16]; pose(one, 0, 0, 0, 0);
  const int rc1 = r3d_posegraph_optimize(1, one, 0, nullptr, nullptr, nullptr, nullptr, 0.05, 1.0, 0.25, 5, nullptr, nullptr);
  std::printf("single node rc %d\n", rc1);
  bad += rc1 != 0;
  nodes[1] = 99;
  const int rc2 = r3d_posegraph_optimize(n, start.data(), (int)unc.size(), nodes.data(), Ts.data(), Ls.data(), unc.data(), 0.05, 1.0, 0.25, 100, w.data(), rep.data());
  std::printf("bad node rc %d\n", rc2);
  bad += rc2 != R3D_ERR_INVALID;
  double s[11] = {7, 1.5, -2.25, 3, 10, 0.5, -0.75, 20, 1.25, 30, 0.28}, info[36], f, r;
  const int rc3 = r3d_information_from_sums(s, 9, info, &f, &r);
  std::printf("info rc %d n %g\n", rc3, info[35]);
  bad += rc3 != 0 || info[35] != 7.0 || info[0] != 50.0;
  std::printf(bad ? "FAILED\n" : "host check OK\n");
  return bad ? 1 : 0;
}
