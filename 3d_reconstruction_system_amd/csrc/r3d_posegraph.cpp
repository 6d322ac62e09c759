// Multiway registration on the host: the information matrix and quality of a registered pair from its 11 pair sums
// (r3d_registration_sums, r3d_reginfo.hip) and pose-graph optimisation -- Levenberg-Marquardt over dense normal equations with
// the closed-form line-process weights of Choi, Zhou and Koltun (CVPR 2015).  Plain fp64 C++, no device code, callable without a
// GPU.  include/r3d.h is the specification; DESIGN.md 4.5s says why the solver lives here and not on the device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "r3d_internal.h"

namespace {

constexpr int kMaxNodes = R3D_POSEGRAPH_MAX_NODES;
constexpr double kStepTol = 1e-10, kCostTol = 1e-14;

// ---- rigid 4x4 (row-major) and SO(3) / SE(3) helpers -------------------------------------------------------------------------
void mul4(const double* A, const double* B, double* C) {   // C = A B for [R t; 0 1]
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
    C[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
  }
  C[12] = C[13] = C[14] = 0.0;
  C[15] = 1.0;
}

void inv4(const double* A, double* B) {   // [R^T, -R^T t]
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) B[4 * r + c] = A[4 * c + r];
    B[4 * r + 3] = -((A[r] * A[3] + A[4 + r] * A[7]) + A[8 + r] * A[11]);
  }
  B[12] = B[13] = B[14] = 0.0;
  B[15] = 1.0;
}

// SO(3) logarithm of the rotation block of a 4x4 through its quaternion (Shepperd's branch): sound at every angle up to pi
void so3_log(const double* T, double* w) {
  const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
  const double tr = r00 + r11 + r22;
  double qw, qx, qy, qz;
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(tr + 1.0);
    qw = 0.25 * s, qx = (r21 - r12) / s, qy = (r02 - r20) / s, qz = (r10 - r01) / s;
  } else if (r00 >= r11 && r00 >= r22) {
    const double s = 2.0 * std::sqrt(1.0 + r00 - r11 - r22);
    qw = (r21 - r12) / s, qx = 0.25 * s, qy = (r01 + r10) / s, qz = (r02 + r20) / s;
  } else if (r11 >= r22) {
    const double s = 2.0 * std::sqrt(1.0 + r11 - r00 - r22);
    qw = (r02 - r20) / s, qx = (r01 + r10) / s, qy = 0.25 * s, qz = (r12 + r21) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + r22 - r00 - r11);
    qw = (r10 - r01) / s, qx = (r02 + r20) / s, qy = (r12 + r21) / s, qz = 0.25 * s;
  }
  if (qw < 0.0) qw = -qw, qx = -qx, qy = -qy, qz = -qz;
  const double n = std::sqrt(qx * qx + qy * qy + qz * qz);
  const double k = n > 0.0 ? 2.0 * std::atan2(n, qw) / n : 0.0;
  w[0] = k * qx, w[1] = k * qy, w[2] = k * qz;
}

// sin(t)/t, (1 - cos t)/t^2, (t - sin t)/t^3
void exp_coefficients(double th, double* a, double* b, double* c) {
  const double t2 = th * th;
  if (th < 1e-2) {
    *a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
    *b = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0));
    *c = 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0));
  } else {
    *a = std::sin(th) / th;
    *b = (1.0 - std::cos(th)) / t2;
    *c = (th - std::sin(th)) / (t2 * th);
  }
}

// SE(3) exponential of d = (w, v): R = I + a W + b W^2, t = (I + b W + c W^2) v with W = [w]x
void se3_exp(const double* d, double* T) {
  const double wx = d[0], wy = d[1], wz = d[2];
  double a, b, c;
  exp_coefficients(std::sqrt(wx * wx + wy * wy + wz * wz), &a, &b, &c);
  const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double W2[9];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) W2[3 * r + k] = (W[3 * r] * W[k] + W[3 * r + 1] * W[3 + k]) + W[3 * r + 2] * W[6 + k];
  for (int r = 0; r < 3; ++r) {
    double t = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double id = r == k ? 1.0 : 0.0;
      T[4 * r + k] = id + a * W[3 * r + k] + b * W2[3 * r + k];
      t += (id + b * W[3 * r + k] + c * W2[3 * r + k]) * d[3 + k];
    }
    T[4 * r + 3] = t;
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
}

// inverse of the left Jacobian of SO(3): log(exp(e) exp(w)) = w + Jl^-1(w) e + O(e^2); Jl^-1 = I - W/2 + k W^2,
// k = (1 - (t/2) cot(t/2)) / t^2
void so3_left_jacobian_inverse(const double* w, double* J) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = std::sqrt(t2);
  const double k = th < 1e-2 ? 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 : (1.0 - 0.5 * th * std::cos(0.5 * th) / std::sin(0.5 * th)) / t2;
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double w2 = (W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c]) + W[3 * r + 2] * W[6 + c];
      J[3 * r + c] = (r == c ? 1.0 : 0.0) - 0.5 * W[3 * r + c] + k * w2;
    }
}

// xi = (w, v) of E = T^-1 Xt^-1 Xs and, with Js != NULL, its derivative by the left perturbation of Xs (6x6 row-major; the
// derivative by Xt's is -Js).  With A = (Xt T)^-1: Js = [[Jl^-1(w) R_A, 0], [[t_A - t_E]x R_A, R_A]].
void edge_residual(const double* Xs, const double* Xt, const double* T, double* xi, double* Js) {
  double M[16], A[16], E[16];
  mul4(Xt, T, M);
  inv4(M, A);
  mul4(A, Xs, E);
  so3_log(E, xi);
  xi[3] = E[3], xi[4] = E[7], xi[5] = E[11];
  if (!Js) return;
  double Ji[9];
  so3_left_jacobian_inverse(xi, Ji);
  const double u[3] = {A[3] - E[3], A[7] - E[7], A[11] - E[11]};
  const double U[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double ra0 = A[c], ra1 = A[4 + c], ra2 = A[8 + c];   // column c of R_A
      Js[6 * r + c] = (Ji[3 * r] * ra0 + Ji[3 * r + 1] * ra1) + Ji[3 * r + 2] * ra2;
      Js[6 * r + 3 + c] = 0.0;
      Js[6 * (3 + r) + c] = (U[3 * r] * ra0 + U[3 * r + 1] * ra1) + U[3 * r + 2] * ra2;
      Js[6 * (3 + r) + 3 + c] = A[4 * r + c];
    }
}

double quad6(const double* L, const double* x) {
  double s = 0.0;
  for (int r = 0; r < 6; ++r) {
    double v = 0.0;
    for (int c = 0; c < 6; ++c) v += L[6 * r + c] * x[c];
    s += x[r] * v;
  }
  return s;
}

// ---- the graph ------------------------------------------------------------------------------------------------------------------
struct Graph {
  int n = 0, m = 0;
  const int32_t* nodes = nullptr;
  const double* T = nullptr;
  const uint8_t* uncertain = nullptr;
  std::vector<double> L;        // [m][36], symmetrised
  std::vector<char> active;     // 0: pruned
  bool robust = false;
  double mu = 0.0;

  double weight(int e, double chi2) const {
    if (!robust || !uncertain[e]) return 1.0;
    const double den = mu + chi2;
    if (!(den > 0.0)) return 1.0;
    const double r = mu / den;
    return r * r;
  }

  // C = sum w chi2 and F = the line-process objective at `poses`; w_out (optional) receives the weights, 0 for pruned edges
  void evaluate(const double* poses, double* C, double* F, double* w_out) const {
    double c = 0.0, f = 0.0;
    for (int e = 0; e < m; ++e) {
      if (w_out) w_out[e] = 0.0;
      if (!active[e]) continue;
      double xi[6];
      edge_residual(poses + 16 * nodes[2 * e], poses + 16 * nodes[2 * e + 1], T + 16 * e, xi, nullptr);
      const double chi2 = quad6(&L[36 * (size_t)e], xi), w = weight(e, chi2);
      c += w * chi2;
      f += (robust && uncertain[e] && mu + chi2 > 0.0) ? mu * chi2 / (mu + chi2) : w * chi2;
      if (w_out) w_out[e] = w;
    }
    if (C) *C = c;
    if (F) *F = f;
  }

  void update_mu(double preference, double max_dist) {
    double sum = 0.0;
    int cnt = 0;
    for (int e = 0; e < m; ++e)
      if (active[e] && uncertain[e]) sum += L[36 * (size_t)e + 35], ++cnt;
    mu = cnt ? preference * (max_dist * max_dist) * (sum / cnt) : 0.0;
  }

  // H (dim x dim, dense, row-major) and g at `poses`, dim = 6 (n - 1)
  void normal_equations(const double* poses, std::vector<double>& H, std::vector<double>& g) const {
    const size_t dim = 6 * (size_t)(n - 1);
    std::fill(H.begin(), H.end(), 0.0);
    std::fill(g.begin(), g.end(), 0.0);
    for (int e = 0; e < m; ++e) {
      if (!active[e]) continue;
      const int s = nodes[2 * e], t = nodes[2 * e + 1];
      double xi[6], J[36], WJ[36], Wx[6], B[36], b[6];
      edge_residual(poses + 16 * s, poses + 16 * t, T + 16 * e, xi, J);
      const double* Le = &L[36 * (size_t)e];
      const double w = weight(e, quad6(Le, xi));
      for (int r = 0; r < 6; ++r) {
        double v = 0.0;
        for (int k = 0; k < 6; ++k) v += Le[6 * r + k] * xi[k];
        Wx[r] = w * v;
        for (int c = 0; c < 6; ++c) {
          double a = 0.0;
          for (int k = 0; k < 6; ++k) a += Le[6 * r + k] * J[6 * k + c];
          WJ[6 * r + c] = w * a;
        }
      }
      for (int r = 0; r < 6; ++r) {
        double v = 0.0;
        for (int k = 0; k < 6; ++k) v += J[6 * k + r] * Wx[k];
        b[r] = v;
        for (int c = 0; c < 6; ++c) {
          double a = 0.0;
          for (int k = 0; k < 6; ++k) a += J[6 * k + r] * WJ[6 * k + c];
          B[6 * r + c] = a;
        }
      }
      // Jt = -Js: the diagonal blocks take +B, the off-diagonal ones -B; node 0 has no parameters
      const size_t os = 6 * (size_t)(s - 1), ot = 6 * (size_t)(t - 1);
      for (int r = 0; r < 6; ++r) {
        if (s) g[os + r] += b[r];
        if (t) g[ot + r] -= b[r];
        for (int c = 0; c < 6; ++c) {
          if (s) H[(os + r) * dim + os + c] += B[6 * r + c];
          if (t) H[(ot + r) * dim + ot + c] += B[6 * r + c];
          if (s && t) {
            H[(os + r) * dim + ot + c] -= B[6 * r + c];
            H[(ot + r) * dim + os + c] -= B[6 * c + r];
          }
        }
      }
    }
  }
};

// A = L L^T in place (lower triangle, row-major); false when A is not positive definite
bool cholesky(std::vector<double>& A, size_t dim) {
  for (size_t i = 0; i < dim; ++i) {
    double* ri = &A[i * dim];
    for (size_t j = 0; j <= i; ++j) {
      const double* rj = &A[j * dim];
      double s = ri[j];
      for (size_t k = 0; k < j; ++k) s -= ri[k] * rj[k];
      if (i == j) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        ri[i] = std::sqrt(s);
      } else {
        ri[j] = s / rj[j];
      }
    }
  }
  return true;
}

void cholesky_solve(const std::vector<double>& Lc, size_t dim, std::vector<double>& x) {   // x <- (L L^T)^-1 x
  for (size_t i = 0; i < dim; ++i) {
    double s = x[i];
    for (size_t k = 0; k < i; ++k) s -= Lc[i * dim + k] * x[k];
    x[i] = s / Lc[i * dim + i];
  }
  for (size_t i = dim; i-- > 0;) {
    double s = x[i];
    for (size_t k = i + 1; k < dim; ++k) s -= Lc[k * dim + i] * x[k];
    x[i] = s / Lc[i * dim + i];
  }
}

// One Levenberg-Marquardt loop over the active edges; returns 1 when it ended because of max_iters
int lm_loop(const Graph& G, std::vector<double>& poses, int max_iters, int* iters) {
  const size_t dim = 6 * (size_t)(G.n - 1);
  double F = 0.0;
  G.evaluate(poses.data(), nullptr, &F, nullptr);
  if (dim == 0) return 0;
  std::vector<double> H(dim * dim), A(dim * dim), g(dim), d(dim), trial(poses.size());
  double lambda = -1.0, nu = 2.0;
  bool fresh = false;
  for (int it = 0; it < max_iters; ++it) {
    if (F == 0.0) return 0;
    if (!fresh) {
      G.normal_equations(poses.data(), H, g);
      fresh = true;
    }
    if (lambda < 0.0) {
      double top = 0.0;
      for (size_t k = 0; k < dim; ++k) top = std::fmax(top, H[k * dim + k]);
      if (!(top > 0.0)) return 0;   // no edge constrains any free node
      lambda = 1e-6 * top;
    }
    ++*iters;
    A = H;
    for (size_t k = 0; k < dim; ++k) A[k * dim + k] += lambda;
    if (!cholesky(A, dim)) {
      lambda *= 10.0;
      if (!std::isfinite(lambda)) return 0;
      continue;
    }
    for (size_t k = 0; k < dim; ++k) d[k] = -g[k];
    cholesky_solve(A, dim, d);
    double dmax = 0.0, pred = 0.0;
    for (size_t k = 0; k < dim; ++k) {
      dmax = std::fmax(dmax, std::fabs(d[k]));
      pred += d[k] * (lambda * d[k] - g[k]);
    }
    trial = poses;
    for (int i = 1; i < G.n; ++i) {
      double X[16];
      se3_exp(&d[6 * (size_t)(i - 1)], X);
      mul4(X, &poses[16 * (size_t)i], &trial[16 * (size_t)i]);
    }
    double Fn = 0.0;
    G.evaluate(trial.data(), nullptr, &Fn, nullptr);
    if (dmax < kStepTol) {
      if (Fn <= F) poses.swap(trial);
      return 0;
    }
    if (Fn < F) {
      const double drop = F - Fn, rho = pred > 0.0 ? drop / pred : 1.0, q = 2.0 * rho - 1.0;
      poses.swap(trial);
      fresh = false;
      lambda *= std::fmax(1.0 / 3.0, 1.0 - q * q * q);
      nu = 2.0;
      const bool flat = drop < kCostTol * F;
      F = Fn;
      if (flat) return 0;
    } else {
      lambda *= nu;
      nu *= 2.0;
      if (!std::isfinite(lambda)) return 0;
    }
  }
  return F == 0.0 ? 0 : 1;
}

bool finite_all(const double* p, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(p[k])) return false;
  return true;
}

bool rigid_bottom_row(const double* T) { return T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0; }

}  // namespace

extern "C" {

int r3d_information_from_sums(const double* h_sums, int64_t n_src, double* h_info, double* h_fitness, double* h_rmse) {
  R3D_REQUIRE(h_sums && h_info, "NULL argument");
  R3D_REQUIRE(n_src >= 0, "negative cloud size");
  const double* s = h_sums;
  const double n = s[0];
  const double I[36] = {s[7] + s[9], -s[5],       -s[6],       0.0,   -s[3], s[2],    //
                        -s[5],       s[4] + s[9], -s[8],       s[3],  0.0,   -s[1],   //
                        -s[6],       -s[8],       s[4] + s[7], -s[2], s[1],  0.0,     //
                        0.0,         s[3],        -s[2],       n,     0.0,   0.0,     //
                        -s[3],       0.0,         s[1],        0.0,   n,     0.0,     //
                        s[2],        -s[1],       0.0,         0.0,   0.0,   n};
  for (int k = 0; k < 36; ++k) h_info[k] = I[k] + 0.0;   // + 0.0: no negative zeros
  if (h_fitness) *h_fitness = n_src > 0 ? n / (double)n_src : 0.0;
  if (h_rmse) *h_rmse = n > 0.0 ? std::sqrt(s[10] / n) : 0.0;
  return R3D_OK;
}

int r3d_posegraph_optimize(int n_nodes, double* h_poses, int n_edges, const int32_t* h_edge_nodes, const double* h_edge_T,
                           const double* h_edge_info, const uint8_t* h_edge_uncertain, double max_correspondence_distance,
                           double preference_loop_closure, double prune_threshold, int max_iters, double* h_edge_weight_out,
                           double* h_report) {
  R3D_REQUIRE(n_nodes >= 1 && n_nodes <= kMaxNodes, "n_nodes must be in [1, %d], got %d", kMaxNodes, n_nodes);
  R3D_REQUIRE(n_edges >= 0 && max_iters >= 0, "negative edge or iteration count");
  R3D_REQUIRE(h_poses != nullptr, "h_poses is NULL");
  R3D_REQUIRE(n_edges == 0 || (h_edge_nodes && h_edge_T && h_edge_info && h_edge_uncertain), "NULL edge array");
  R3D_REQUIRE(std::isfinite(max_correspondence_distance) && max_correspondence_distance > 0.0,
              "max_correspondence_distance must be finite and > 0");
  R3D_REQUIRE(preference_loop_closure > 0.0, "preference_loop_closure must be > 0 (+inf: no robust weights)");
  R3D_REQUIRE(std::isfinite(prune_threshold), "prune_threshold must be finite");
  R3D_REQUIRE(finite_all(h_poses, 16 * (size_t)n_nodes), "a pose holds a non-finite value");
  for (int i = 0; i < n_nodes; ++i) R3D_REQUIRE(rigid_bottom_row(h_poses + 16 * (size_t)i), "the bottom row of pose %d is not 0 0 0 1", i);

  Graph G;
  G.n = n_nodes, G.m = n_edges, G.nodes = h_edge_nodes, G.T = h_edge_T, G.uncertain = h_edge_uncertain;
  G.L.resize(36 * (size_t)n_edges);
  G.active.assign((size_t)n_edges, 1);
  for (int e = 0; e < n_edges; ++e) {
    const int s = h_edge_nodes[2 * e], t = h_edge_nodes[2 * e + 1];
    R3D_REQUIRE(s >= 0 && s < n_nodes && t >= 0 && t < n_nodes && s != t, "edge %d joins nodes %d and %d of %d", e, s, t, n_nodes);
    const double *Te = h_edge_T + 16 * (size_t)e, *Le = h_edge_info + 36 * (size_t)e;
    R3D_REQUIRE(finite_all(Te, 16) && finite_all(Le, 36), "edge %d holds a non-finite value", e);
    R3D_REQUIRE(rigid_bottom_row(Te), "the bottom row of the T of edge %d is not 0 0 0 1", e);
    double top = 0.0;
    for (int k = 0; k < 36; ++k) top = std::fmax(top, std::fabs(Le[k]));
    for (int r = 0; r < 6; ++r) {
      R3D_REQUIRE(Le[7 * r] >= 0.0, "the information matrix of edge %d has a negative diagonal entry", e);
      for (int c = 0; c < 6; ++c) {
        R3D_REQUIRE(std::fabs(Le[6 * r + c] - Le[6 * c + r]) <= 1e-9 * top, "the information matrix of edge %d is not symmetric", e);
        G.L[36 * (size_t)e + 6 * r + c] = 0.5 * (Le[6 * r + c] + Le[6 * c + r]);
      }
    }
  }
  {   // every node must hang on node 0
    std::vector<char> seen((size_t)n_nodes, 0);
    std::vector<int> todo(1, 0);
    seen[0] = 1;
    while (!todo.empty()) {
      const int a = todo.back();
      todo.pop_back();
      for (int e = 0; e < n_edges; ++e) {
        const int s = h_edge_nodes[2 * e], t = h_edge_nodes[2 * e + 1], b = s == a ? t : t == a ? s : -1;
        if (b >= 0 && !seen[b]) seen[b] = 1, todo.push_back(b);
      }
    }
    for (int i = 0; i < n_nodes; ++i) R3D_REQUIRE(seen[i], "no path of edges connects node %d to node 0", i);
  }

  G.robust = std::isfinite(preference_loop_closure);
  if (G.robust) G.update_mu(preference_loop_closure, max_correspondence_distance);
  std::vector<double> poses(h_poses, h_poses + 16 * (size_t)n_nodes);
  double c0 = 0.0, c1 = 0.0;
  G.evaluate(poses.data(), &c0, nullptr, nullptr);
  int iters = 0, pruned = 0;
  int status = lm_loop(G, poses, max_iters, &iters);
  std::vector<double> w((size_t)n_edges);
  G.evaluate(poses.data(), &c1, nullptr, w.data());
  if (G.robust) {
    for (int e = 0; e < n_edges; ++e)
      if (h_edge_uncertain[e] && w[e] < prune_threshold) G.active[e] = 0, ++pruned;
    if (pruned) {
      G.update_mu(preference_loop_closure, max_correspondence_distance);
      status |= lm_loop(G, poses, max_iters, &iters);
      G.evaluate(poses.data(), &c1, nullptr, w.data());
    }
  }
  for (size_t k = 16; k < poses.size(); ++k) h_poses[k] = poses[k];   // node 0 keeps its bits
  if (h_edge_weight_out)
    for (int e = 0; e < n_edges; ++e) h_edge_weight_out[e] = w[e];
  if (h_report) {
    for (int k = 0; k < R3D_POSEGRAPH_REPORT_DOUBLES; ++k) h_report[k] = 0.0;
    h_report[0] = c0, h_report[1] = c1, h_report[2] = (double)iters, h_report[3] = (double)pruned, h_report[4] = (double)status;
  }
  return R3D_OK;
}

}  // extern "C"
