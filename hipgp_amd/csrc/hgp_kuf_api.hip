// hgp_kuf_api.hip — the extern "C" entries of the observation-side family (see include/hipgp.h): the cross
// covariances hgp_kuf_*, their gradients, the products and their windowed twins, hgp_knn_doubly_diag and the
// Fourier-feature products hgp_rff_*.  Pure argument plumbing: an entry fills one KufObs (hgp_internal.hpp), names
// the rules that apply to it and calls its launcher.  Every rule of the hgp_kuf_* entries is written once, with its
// message once; the RFF and doubly-diag entries keep their own rules and wording in their own bodies (they share
// rule_dtype, rule_sizes and the epilogue).  Every rule runs before any HIP call.  DESIGN.md section 29 has the
// table of which entry applies which rule.
#include <cmath>
#include <string>

#include "../../include/hipgp.h"
#include "hgp_internal.hpp"

using namespace hgp;

namespace {

// a rule's third outcome beside 0 (go on) and an error (< 0): a valid call with nothing to do
constexpr int KUF_EMPTY = 1;

// An entry: `checks` (rules through HGP_TRY, in the entry's order), then `launch`; the one place that turns
// KUF_EMPTY into success and a HIP error into HGP_E_HIP under the entry's name.
template <typename C, typename L>
int kuf_call(const char* name, C&& checks, L&& launch) {
  const int c = checks();
  if (c != 0) return c == KUF_EMPTY ? 0 : c;
  const hipError_t e = launch();
  if (e != hipSuccess) return fail(HGP_E_HIP, std::string(name) + ": " + hipGetErrorString(e));
  return 0;
}

void set3(double* v, double a) { v[0] = v[1] = v[2] = a; }

// the record of a scalar entry (ell, rho on every axis); an _ard entry passes 0 and lets rule_ard fill them
KufObs kuf_obs(int dtype, int mode, int kind, double kp, int ndim, const int64_t* m, const void* const* grids,
               const void* x, int64_t nobs, double sig2, double ell, void* hip_stream, double rho = 0, int npts = 0,
               const void* u = nullptr, const int* pieces = nullptr) {
  KufObs o;
  o.dtype = dtype, o.mode = mode, o.kind = kind, o.kp = kp;
  o.ndim = ndim, o.m = m, o.grids = grids, o.x = x, o.nobs = nobs, o.sig2 = sig2;
  set3(o.ell, ell);
  set3(o.rho, rho);
  o.npts = npts, o.u = u, o.pieces = pieces;
  o.stream = reinterpret_cast<hipStream_t>(hip_stream);
  return o;
}

// ---- the rules ----
int rule_dtype(int dtype) {
  if (dtype != HGP_F32 && dtype != HGP_F64) return fail(HGP_E_ARG, "dtype must be HGP_F32 or HGP_F64");
  return 0;
}

int rule_grid(const KufObs& o) {
  if (o.ndim < 1 || o.ndim > 3 || o.m == nullptr || o.grids == nullptr)
    return fail(HGP_E_ARG, "ndim must be 1..3, m/grids non-null");
  return 0;
}

// after rule_grid
int rule_sizes(int ndim, const int64_t* m, const void* const* grids) {
  for (int a = 0; a < ndim; ++a)
    if (m[a] < 1 || grids[a] == nullptr) return fail(HGP_E_ARG, "grid sizes must be >= 1 with non-null grids");
  return 0;
}

int rule_kind(const KufObs& o, int last) {
  if (o.kind < HGP_KERN_SQEXP || o.kind > last) return fail(HGP_E_ARG, "bad kernel kind");
  return 0;
}

// the kernel by mode: point observations up to Matern 5/2; semi-mc up to Gneiting, with npts in [1, 1024] and the
// offset draw; semi-sqexp has no choice
int rule_kernel(const KufObs& o) {
  HGP_TRY(rule_kind(o, o.mode == 1 ? HGP_KERN_GNEITING : HGP_KERN_MATERN52));
  if (o.mode != 1) return 0;
  if (o.npts < 1 || o.npts > 1024) return fail(HGP_E_ARG, "npts must be in [1, 1024]");
  if (o.u == nullptr) return fail(HGP_E_ARG, "u (the device offset draw) is null");
  return 0;
}

// the windowed entries: no Gneiting, and a scalar entry's rho (an _ard entry's: rule_ard)
int rule_win(const KufObs& o) {
  HGP_TRY(rule_kind(o, HGP_KERN_MATERN52));
  if (!(o.rho[0] >= 0) || !std::isfinite(o.rho[0])) return fail(HGP_E_ARG, "rho must be finite and >= 0");
  return 0;
}

// The _ard entries, ahead of their scalar twins' rules (ell and rho hold ndim values): SqExp, every ell[a] finite
// and > 0, every rho[a] finite and >= 0 (want_rho: the windowed entries).  Fills o.ell / o.rho, the last value
// repeated on the absent axes.
int rule_ard(KufObs& o, const double* ell, const double* rho = nullptr, bool want_rho = false) {
  HGP_TRY(rule_grid(o));
  if (o.kind != HGP_KERN_SQEXP) return fail(HGP_E_ARG, "a length scale per axis is defined for HGP_KERN_SQEXP only");
  if (ell == nullptr || (want_rho && rho == nullptr)) return fail(HGP_E_ARG, "null ell / rho");
  for (int a = 0; a < o.ndim; ++a) {
    if (!(ell[a] > 0) || !std::isfinite(ell[a])) return fail(HGP_E_ARG, "every ell[a] must be finite and > 0");
    if (want_rho && (!(rho[a] >= 0) || !std::isfinite(rho[a])))
      return fail(HGP_E_ARG, "every rho[a] must be finite and >= 0");
  }
  for (int a = 0; a < 3; ++a) {
    o.ell[a] = ell[a < o.ndim ? a : o.ndim - 1];
    if (want_rho) o.rho[a] = rho[a < o.ndim ? a : o.ndim - 1];
  }
  return 0;
}

int rule_pieces(const KufObs& o, int64_t npieces) {
  if (npieces != o.nobs) return fail(HGP_E_ARG, "pieces must hold nobs entries");
  if (o.nobs > 0 && o.pieces == nullptr) return fail(HGP_E_ARG, "null pieces");
  return 0;
}

// rows: "nw" or "nc"
int rule_counts(const KufObs& o, const char* rows, int64_t n, int64_t nsplit) {
  if (o.nobs < 0 || n < 0 || nsplit < 0)
    return fail(HGP_E_ARG, std::string("nobs, ") + rows + " and nsplit must be >= 0");
  return 0;
}

// ---- the rules of one product, in order; each holds the product's null-pointer rule and its empty outcome ----
// the forwards: hgp_kuf_grid(_ard) returns on nobs = 0 before the grids are looked at, the semi forwards after
// (both kept as they were: DESIGN.md section 29)
int rules_fwd(const KufObs& o, const void* out) {
  HGP_TRY(rule_grid(o));
  HGP_TRY(rule_kernel(o));
  HGP_TRY(rule_dtype(o.dtype));
  if (o.mode == 0 && o.nobs == 0) return KUF_EMPTY;
  if (o.nobs < 0 || (o.nobs > 0 && (o.x == nullptr || out == nullptr))) return fail(HGP_E_ARG, "bad x/out/nobs");
  HGP_TRY(rule_sizes(o.ndim, o.m, o.grids));
  return o.nobs == 0 ? KUF_EMPTY : 0;
}

// the gradients: every kernel code passes the range and Gneiting is refused last, as unsupported; nobs = 0 goes on
// to the launcher, which zeroes grad2
int rules_grad(const KufObs& o, const void* g, const void* grad2) {
  if (o.mode == 1) HGP_TRY(rule_kernel(o));
  HGP_TRY(rule_grid(o));
  HGP_TRY(rule_dtype(o.dtype));
  HGP_TRY(rule_kind(o, HGP_KERN_GNEITING));
  if (grad2 == nullptr) return fail(HGP_E_ARG, "grad2 is null");
  if (o.nobs < 0 || (o.nobs > 0 && (o.x == nullptr || g == nullptr))) return fail(HGP_E_ARG, "bad x/g/nobs");
  HGP_TRY(rule_sizes(o.ndim, o.m, o.grids));
  if (o.kind == HGP_KERN_GNEITING)
    return fail(HGP_E_UNSUPPORTED, "no hyper-parameter gradient for the Gneiting kernel (the reference's is NaN at r = 0)");
  return 0;
}

// what the products and the transposed products share up to their empty outcome; rows: "nw" or "nc"
int rules_product(const KufObs& o, const char* rows, int64_t n, int64_t nsplit) {
  HGP_TRY(rule_kernel(o));
  HGP_TRY(rule_grid(o));
  HGP_TRY(rule_dtype(o.dtype));
  HGP_TRY(rule_counts(o, rows, n, nsplit));
  return rule_sizes(o.ndim, o.m, o.grids);
}

// the products: nobs = 0 or nw = 0 is empty, nothing written
int rules_matvec(const KufObs& o, const void* w, int64_t nw, int64_t nsplit, const void* out) {
  HGP_TRY(rules_product(o, "nw", nw, nsplit));
  if (o.nobs == 0 || nw == 0) return KUF_EMPTY;
  if (o.x == nullptr || w == nullptr || out == nullptr) return fail(HGP_E_ARG, "null x / w / out");
  return 0;
}

// the transposed products: nc = 0 is empty; nobs = 0 goes on to the launcher, which zeroes out
int rules_rmatvec(const KufObs& o, const void* c, int64_t nc, int64_t nsplit, const void* out) {
  HGP_TRY(rules_product(o, "nc", nc, nsplit));
  if (nc == 0) return KUF_EMPTY;
  if (out == nullptr || (o.nobs > 0 && (o.x == nullptr || c == nullptr))) return fail(HGP_E_ARG, "null x / c / out");
  return 0;
}

int rules_rmatvec_win(const KufObs& o, const void* c, int64_t nc, const int64_t* order, const int64_t* bin_start,
                      const void* out) {
  HGP_TRY(rules_rmatvec(o, c, nc, 0, out));
  if (o.nobs > 0 && (order == nullptr || bin_start == nullptr)) return fail(HGP_E_ARG, "null order / bin_start");
  return 0;
}

// the windowed line integrals, ahead of the product's own rules: the window, then the piece counts
int rules_line_win(const KufObs& o, int64_t npieces) {
  HGP_TRY(rule_win(o));
  return rule_pieces(o, npieces);
}

}  // namespace

extern "C" {

// ---- the dense cross covariances ----
int hgp_kuf_grid(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                 int64_t nobs, double sig2, double ell, void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_grid", [&] { return rules_fwd(o, out); }, [&] { return kuf_grid(o, out); });
}

int hgp_kuf_grid_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                     int64_t nobs, double sig2, const double* ell, void* out, void* hip_stream) {
  KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, 0, hip_stream);
  return kuf_call("hgp_kuf_grid_ard", [&] { HGP_TRY(rule_ard(o, ell)); return rules_fwd(o, out); },
                  [&] { return kuf_grid(o, out); });
}

int hgp_kuf_semi_mc(int dtype, int kind, double kparam, int ndim, const int64_t* m, const void* const* grids,
                    const void* x, int64_t nobs, double sig2, double ell, int npts, const void* u, void* out,
                    void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 1, kind, kparam, ndim, m, grids, x, nobs, sig2, ell, hip_stream, 0, npts, u);
  return kuf_call("hgp_kuf_semi_mc", [&] { return rules_fwd(o, out); }, [&] { return kuf_semi(o, out); });
}

int hgp_kuf_semi_sqexp(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x, int64_t nobs,
                       double sig2, double ell, void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 2, HGP_KERN_SQEXP, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_semi_sqexp", [&] { return rules_fwd(o, out); }, [&] { return kuf_semi(o, out); });
}

// ---- their (sig2, ell) backward ----
int hgp_kuf_grid_grad(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                      int64_t nobs, double sig2, double ell, const void* g, void* grad2, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_grid_grad", [&] { return rules_grad(o, g, grad2); }, [&] { return kuf_grad(o, g, grad2); });
}

int hgp_kuf_grid_grad_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                          int64_t nobs, double sig2, const double* ell, const void* g, void* grad, void* hip_stream) {
  KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, 0, hip_stream);
  return kuf_call("hgp_kuf_grid_grad_ard", [&] { HGP_TRY(rule_ard(o, ell)); return rules_grad(o, g, grad); },
                  [&] { return kuf_grad_ard(o, g, grad); });
}

int hgp_kuf_semi_mc_grad(int dtype, int kind, double kparam, int ndim, const int64_t* m, const void* const* grids,
                         const void* x, int64_t nobs, double sig2, double ell, int npts, const void* u,
                         const void* g, void* grad2, void* hip_stream) {
  // kparam is Gneiting's alpha, and that kernel is refused: the record keeps it all the same
  const KufObs o = kuf_obs(dtype, 1, kind, kparam, ndim, m, grids, x, nobs, sig2, ell, hip_stream, 0, npts, u);
  return kuf_call("hgp_kuf_semi_mc_grad", [&] { return rules_grad(o, g, grad2); },
                  [&] { return kuf_grad(o, g, grad2); });
}

int hgp_kuf_semi_sqexp_grad(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                            int64_t nobs, double sig2, double ell, const void* g, void* grad2, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 2, HGP_KERN_SQEXP, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_semi_sqexp_grad", [&] { return rules_grad(o, g, grad2); },
                  [&] { return kuf_grad(o, g, grad2); });
}

// ---- the products Kuf w^T ----
int hgp_kuf_grid_matvec(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                        int64_t nobs, double sig2, double ell, const void* w, int64_t nw, int64_t nsplit, void* out,
                        void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_grid_matvec", [&] { return rules_matvec(o, w, nw, nsplit, out); },
                  [&] { return kuf_matvec(o, w, nw, nsplit, out); });
}

int hgp_kuf_grid_matvec_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                            int64_t nobs, double sig2, const double* ell, const void* w, int64_t nw, int64_t nsplit,
                            void* out, void* hip_stream) {
  KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, 0, hip_stream);
  return kuf_call("hgp_kuf_grid_matvec_ard",
                  [&] { HGP_TRY(rule_ard(o, ell)); return rules_matvec(o, w, nw, nsplit, out); },
                  [&] { return kuf_matvec(o, w, nw, nsplit, out); });
}

int hgp_kuf_semi_mc_matvec(int dtype, int kind, double kparam, int ndim, const int64_t* m, const void* const* grids,
                           const void* x, int64_t nobs, double sig2, double ell, int npts, const void* u,
                           const void* w, int64_t nw, int64_t nsplit, void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 1, kind, kparam, ndim, m, grids, x, nobs, sig2, ell, hip_stream, 0, npts, u);
  return kuf_call("hgp_kuf_semi_mc_matvec", [&] { return rules_matvec(o, w, nw, nsplit, out); },
                  [&] { return kuf_matvec(o, w, nw, nsplit, out); });
}

int hgp_kuf_semi_sqexp_matvec(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                              int64_t nobs, double sig2, double ell, const void* w, int64_t nw, int64_t nsplit,
                              void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 2, HGP_KERN_SQEXP, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_semi_sqexp_matvec", [&] { return rules_matvec(o, w, nw, nsplit, out); },
                  [&] { return kuf_matvec(o, w, nw, nsplit, out); });
}

// ---- the transposed products c Kuf ----
int hgp_kuf_grid_rmatvec(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                         int64_t nobs, double sig2, double ell, const void* c, int64_t nc, int64_t nsplit, void* out,
                         void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_grid_rmatvec", [&] { return rules_rmatvec(o, c, nc, nsplit, out); },
                  [&] { return kuf_rmatvec(o, c, nc, nsplit, out); });
}

int hgp_kuf_grid_rmatvec_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                             int64_t nobs, double sig2, const double* ell, const void* c, int64_t nc, int64_t nsplit,
                             void* out, void* hip_stream) {
  KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, 0, hip_stream);
  return kuf_call("hgp_kuf_grid_rmatvec_ard",
                  [&] { HGP_TRY(rule_ard(o, ell)); return rules_rmatvec(o, c, nc, nsplit, out); },
                  [&] { return kuf_rmatvec(o, c, nc, nsplit, out); });
}

int hgp_kuf_semi_mc_rmatvec(int dtype, int kind, double kparam, int ndim, const int64_t* m, const void* const* grids,
                            const void* x, int64_t nobs, double sig2, double ell, int npts, const void* u,
                            const void* c, int64_t nc, int64_t nsplit, void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 1, kind, kparam, ndim, m, grids, x, nobs, sig2, ell, hip_stream, 0, npts, u);
  return kuf_call("hgp_kuf_semi_mc_rmatvec", [&] { return rules_rmatvec(o, c, nc, nsplit, out); },
                  [&] { return kuf_rmatvec(o, c, nc, nsplit, out); });
}

int hgp_kuf_semi_sqexp_rmatvec(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                               int64_t nobs, double sig2, double ell, const void* c, int64_t nc, int64_t nsplit,
                               void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 2, HGP_KERN_SQEXP, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream);
  return kuf_call("hgp_kuf_semi_sqexp_rmatvec", [&] { return rules_rmatvec(o, c, nc, nsplit, out); },
                  [&] { return kuf_rmatvec(o, c, nc, nsplit, out); });
}

// ---- the point products over a window ----
int hgp_kuf_grid_matvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                            int64_t nobs, double sig2, double ell, double rho, const void* w, int64_t nw, void* out,
                            void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream, rho);
  return kuf_call("hgp_kuf_grid_matvec_win", [&] { HGP_TRY(rule_win(o)); return rules_matvec(o, w, nw, 0, out); },
                  [&] { return kuf_matvec_win(o, w, nw, out); });
}

int hgp_kuf_grid_matvec_win_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                                const void* x, int64_t nobs, double sig2, const double* ell, const double* rho,
                                const void* w, int64_t nw, void* out, void* hip_stream) {
  KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, 0, hip_stream);
  return kuf_call("hgp_kuf_grid_matvec_win_ard",
                  [&] { HGP_TRY(rule_ard(o, ell, rho, true)); return rules_matvec(o, w, nw, 0, out); },
                  [&] { return kuf_matvec_win(o, w, nw, out); });
}

int hgp_kuf_grid_rmatvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids, const void* x,
                             int64_t nobs, double sig2, double ell, double rho, const void* c, int64_t nc,
                             const int64_t* order, const int64_t* bin_start, void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream, rho);
  return kuf_call("hgp_kuf_grid_rmatvec_win",
                  [&] { HGP_TRY(rule_win(o)); return rules_rmatvec_win(o, c, nc, order, bin_start, out); },
                  [&] { return kuf_rmatvec_win(o, c, nc, order, bin_start, out); });
}

int hgp_kuf_grid_rmatvec_win_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                                 const void* x, int64_t nobs, double sig2, const double* ell, const double* rho,
                                 const void* c, int64_t nc, const int64_t* order, const int64_t* bin_start, void* out,
                                 void* hip_stream) {
  KufObs o = kuf_obs(dtype, 0, kind, 1.0, ndim, m, grids, x, nobs, sig2, 0, hip_stream);
  return kuf_call("hgp_kuf_grid_rmatvec_win_ard",
                  [&] {
                    HGP_TRY(rule_ard(o, ell, rho, true));
                    return rules_rmatvec_win(o, c, nc, order, bin_start, out);
                  },
                  [&] { return kuf_rmatvec_win(o, c, nc, order, bin_start, out); });
}

int hgp_kuf_win_bins(int ndim, const int64_t* m, int64_t* tile_out, int64_t* nbins_out) {
  if (ndim < 1 || ndim > 3 || m == nullptr) return fail(HGP_E_ARG, "ndim must be 1..3, m non-null");
  if (tile_out == nullptr || nbins_out == nullptr) return fail(HGP_E_ARG, "null tile_out / nbins_out");
  for (int a = 0; a < ndim; ++a)
    if (m[a] < 1) return fail(HGP_E_ARG, "grid sizes must be >= 1");
  kuf_win_geometry(ndim, m, tile_out, nbins_out);
  return 0;
}

// ---- the line-integral products over the window of a line ----
int hgp_kuf_semi_mc_matvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                               const void* x, int64_t nobs, double sig2, double ell, double rho, int npts,
                               const void* u, const int* pieces, int64_t npieces, const void* w, int64_t nw,
                               void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 1, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream, rho, npts, u, pieces);
  return kuf_call("hgp_kuf_semi_mc_matvec_win",
                  [&] { HGP_TRY(rules_line_win(o, npieces)); return rules_matvec(o, w, nw, 0, out); },
                  [&] { return kuf_line_matvec_win(o, w, nw, out); });
}

int hgp_kuf_semi_sqexp_matvec_win(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                                  int64_t nobs, double sig2, double ell, double rho, const int* pieces,
                                  int64_t npieces, const void* w, int64_t nw, void* out, void* hip_stream) {
  const KufObs o =
      kuf_obs(dtype, 2, HGP_KERN_SQEXP, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream, rho, 0, nullptr, pieces);
  return kuf_call("hgp_kuf_semi_sqexp_matvec_win",
                  [&] { HGP_TRY(rules_line_win(o, npieces)); return rules_matvec(o, w, nw, 0, out); },
                  [&] { return kuf_line_matvec_win(o, w, nw, out); });
}

int hgp_kuf_semi_mc_rmatvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                                const void* x, int64_t nobs, double sig2, double ell, double rho, int npts,
                                const void* u, const int* pieces, int64_t npieces, const void* c, int64_t nc,
                                void* out, void* hip_stream) {
  const KufObs o = kuf_obs(dtype, 1, kind, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream, rho, npts, u, pieces);
  return kuf_call("hgp_kuf_semi_mc_rmatvec_win",
                  [&] { HGP_TRY(rules_line_win(o, npieces)); return rules_rmatvec(o, c, nc, 0, out); },
                  [&] { return kuf_line_rmatvec_win(o, c, nc, out); });
}

int hgp_kuf_semi_sqexp_rmatvec_win(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                                   int64_t nobs, double sig2, double ell, double rho, const int* pieces,
                                   int64_t npieces, const void* c, int64_t nc, void* out, void* hip_stream) {
  const KufObs o =
      kuf_obs(dtype, 2, HGP_KERN_SQEXP, 1.0, ndim, m, grids, x, nobs, sig2, ell, hip_stream, rho, 0, nullptr, pieces);
  return kuf_call("hgp_kuf_semi_sqexp_rmatvec_win",
                  [&] { HGP_TRY(rules_line_win(o, npieces)); return rules_rmatvec(o, c, nc, 0, out); },
                  [&] { return kuf_line_rmatvec_win(o, c, nc, out); });
}

// ---- the Fourier-feature products and the doubly-integrated diagonal: rules of their own, the same epilogue ----
int hgp_rff_matvec(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x, int64_t nobs,
                   const void* omega, const void* phase, int64_t nfeat, const void* w, int64_t nw, double scale,
                   int transposed, double beta, int64_t nsplit, void* out, void* hip_stream) {
  int64_t npoints = nobs;
  return kuf_call(
      "hgp_rff_matvec",
      [&] {
        if (ndim < 1 || ndim > 3) return fail(HGP_E_ARG, "ndim must be 1..3");
        HGP_TRY(rule_dtype(dtype));
        if ((x == nullptr) == (grids == nullptr))
          return fail(HGP_E_ARG, "the points are either x (explicit rows) or grids (the mesh): give exactly one");
        if (nobs < 0 || nfeat < 0 || nw < 0 || nsplit < 0)
          return fail(HGP_E_ARG, "nobs, nfeat, nw and nsplit must be >= 0");
        if (x == nullptr) {
          if (m == nullptr) return fail(HGP_E_ARG, "mesh mode needs m");
          HGP_TRY(rule_sizes(ndim, m, grids));
          npoints = 1;
          for (int a = 0; a < ndim; ++a) npoints *= m[a];
        }
        if (npoints == 0 || nw == 0) return KUF_EMPTY;
        if (nfeat < 1) return fail(HGP_E_ARG, "nfeat must be >= 1 when there are points");
        if (omega == nullptr || phase == nullptr || w == nullptr || out == nullptr)
          return fail(HGP_E_ARG, "null omega / phase / w / out");
        return 0;
      },
      [&] {
        return rff_matvec(dtype, ndim, m, grids, x, npoints, omega, phase, nfeat, w, nw, scale, transposed != 0, beta,
                          nsplit, out, reinterpret_cast<hipStream_t>(hip_stream));
      });
}

int hgp_rff_line_matvec(int dtype, int ndim, const void* x, int64_t nobs, const void* omega, const void* phase,
                        int64_t nfeat, const void* w, int64_t nw, double scale, int transposed, double beta,
                        int64_t nsplit, void* out, void* hip_stream) {
  return kuf_call(
      "hgp_rff_line_matvec",
      [&] {
        if (ndim < 1 || ndim > 3) return fail(HGP_E_ARG, "ndim must be 1..3");
        HGP_TRY(rule_dtype(dtype));
        if (x == nullptr) return fail(HGP_E_ARG, "null x: the lines are explicit rows (no mesh mode)");
        if (nobs < 0 || nfeat < 0 || nw < 0 || nsplit < 0)
          return fail(HGP_E_ARG, "nobs, nfeat, nw and nsplit must be >= 0");
        if (nobs == 0 || nw == 0) return KUF_EMPTY;
        if (nfeat < 1) return fail(HGP_E_ARG, "nfeat must be >= 1 when there are lines");
        if (omega == nullptr || phase == nullptr || w == nullptr || out == nullptr)
          return fail(HGP_E_ARG, "null omega / phase / w / out");
        return 0;
      },
      [&] {
        return rff_line_matvec(dtype, ndim, x, nobs, omega, phase, nfeat, w, nw, scale, transposed != 0, beta, nsplit,
                               out, reinterpret_cast<hipStream_t>(hip_stream));
      });
}

int hgp_knn_doubly_diag(int dtype, int ndim, const void* x, int64_t nobs, double sig2, double ell, const void* table,
                        int N, void* out, void* hip_stream) {
  return kuf_call(
      "hgp_knn_doubly_diag",
      [&] {
        if (ndim < 1 || ndim > 3) return fail(HGP_E_ARG, "ndim must be 1..3");
        HGP_TRY(rule_dtype(dtype));
        if (N < 2 || table == nullptr) return fail(HGP_E_ARG, "table needs N >= 2 entries");
        if (nobs < 0 || (nobs > 0 && (x == nullptr || out == nullptr))) return fail(HGP_E_ARG, "bad x/out/nobs");
        return nobs == 0 ? KUF_EMPTY : 0;
      },
      [&] {
        return doubly_diag(dtype, ndim, x, nobs, sig2, ell, table, N, out, reinterpret_cast<hipStream_t>(hip_stream));
      });
}

}  // extern "C"
