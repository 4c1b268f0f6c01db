// api_nuisance.hip -- linear nuisance (foreground) modes with a flat prior, integrated out of the likelihood record's
// reductions (include/v21.h: v21_nuisance_whiten, v21_mlp_set_nuisance, v21_mlp_nuisance_info, v21_mlp_nuisance_coef).
// The host side orthonormalises the basis under the record's weights in float64 and projects the record's data once
// (float32 cannot form r^T W r - |b|^2 from data that carry the foreground); the reductions of a handle with a nuisance
// record (loglike, fisher, fit, sample) then run jac_reduce_kernel's NK > 0 instantiations (reduce_kernels.h; reduce_run
// of api_jacobian.hip), and a caller's data matrix is projected by nuis_project_kernel (nuisance_kernels.h) once per call.
#include "api_internal.h"
#include "nuisance_kernels.h"

// Q (K, out) and R (K, K, upper triangular, row-major) with Q W Q^T = I and sqrt(W) A^T = (sqrt(W) Q^T) R: modified
// Gram-Schmidt, applied twice, on the rows sqrt(w) A_j / |sqrt(w) A_j| (a Cholesky factor of A W A^T would square the
// basis' condition number).  Q is zero on the bins with w == 0.
extern "C" int v21_nuisance_whiten(const double* basis, const float* inv_var, int32_t n_modes, int32_t out_dim, double* q, double* r) {
  if (!basis || !inv_var || !q || !r) return fail(V21_ERR_ARG, "null argument");
  if (n_modes < 1 || n_modes > kNuisMaxModes) return fail(V21_ERR_ARG, "nuisance: %d modes (1 .. %d)", (int)n_modes, kNuisMaxModes);
  if (out_dim < 1) return fail(V21_ERR_ARG, "nuisance: out_dim %d", (int)out_dim);
  const int K = n_modes, D = out_dim;
  int live = 0;
  for (int k = 0; k < D; ++k) {
    if (!(inv_var[k] >= 0.f) || !std::isfinite(inv_var[k])) return fail(V21_ERR_ARG, "nuisance: inv_var[%d] = %g", k, (double)inv_var[k]);
    live += inv_var[k] > 0.f;
  }
  if (live < K + 1) return fail(V21_ERR_ARG, "nuisance: %d modes on %d bins with weight", K, live);
  std::vector<double> sw(D), v((size_t)K * D), norm(K), rt((size_t)K * K, 0.0);
  for (int k = 0; k < D; ++k) sw[k] = std::sqrt((double)inv_var[k]);
  for (int j = 0; j < K; ++j) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) {
      const double a = sw[k] == 0.0 ? 0.0 : sw[k] * basis[(size_t)j * D + k];
      if (!std::isfinite(a)) return fail(V21_ERR_ARG, "nuisance: basis[%d, %d] = %g", j, k, basis[(size_t)j * D + k]);
      v[(size_t)j * D + k] = a;
      s += a * a;
    }
    norm[j] = std::sqrt(s);
    if (!(norm[j] > 0.0) || !std::isfinite(norm[j])) return fail(V21_ERR_ARG, "nuisance: mode %d vanishes on the bins with weight", j);
    for (int k = 0; k < D; ++k) v[(size_t)j * D + k] /= norm[j];
  }
  for (int j = 0; j < K; ++j) {
    double* vj = &v[(size_t)j * D];
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < j; ++i) {
        const double* qi = &v[(size_t)i * D];
        double c = 0.0;
        for (int k = 0; k < D; ++k) c += qi[k] * vj[k];
        for (int k = 0; k < D; ++k) vj[k] -= c * qi[k];
        rt[(size_t)i * K + j] += c;
      }
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += vj[k] * vj[k];
    s = std::sqrt(s);
    if (!(s >= 1e-10)) return fail(V21_ERR_ARG, "nuisance: mode %d depends on the modes before it (%.3g of its norm is left)", j, s);
    rt[(size_t)j * K + j] = s;
    for (int k = 0; k < D; ++k) vj[k] /= s;
  }
  for (int j = 0; j < K; ++j)
    for (int k = 0; k < D; ++k) q[(size_t)j * D + k] = sw[k] == 0.0 ? 0.0 : v[(size_t)j * D + k] / sw[k];
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) r[(size_t)i * K + j] = rt[(size_t)i * K + j] * norm[j];
  return V21_OK;
}

int nuis_build(const double* basis, const float* w, const float* d, int k, int dout, NuisRecord& rec) {
  if (k < 1 || k > kNuisMaxModes) return fail(V21_ERR_ARG, "nuisance: %d modes (1 .. %d)", k, kNuisMaxModes);  // (before anything is sized by it)
  rec.q.assign((size_t)k * dout, 0.0);
  rec.r.assign((size_t)k * k, 0.0);
  CHK(v21_nuisance_whiten(basis, w, k, dout, rec.q.data(), rec.r.data()));
  rec.cd.assign(k, 0.0);
  for (int j = 0; j < k; ++j) {
    double c = 0.0;
    for (int i = 0; i < dout; ++i)
      if (w[i] != 0.f) c += rec.q[(size_t)j * dout + i] * ((double)w[i] * (double)d[i]);
    rec.cd[j] = c;
  }
  rec.qf.resize((size_t)k * dout);
  for (size_t i = 0; i < rec.qf.size(); ++i) rec.qf[i] = (float)rec.q[i];
  rec.proj.resize(dout);
  for (int i = 0; i < dout; ++i) {
    double v = (double)d[i];
    for (int j = 0; j < k; ++j) v -= rec.q[(size_t)j * dout + i] * rec.cd[j];
    rec.proj[i] = (float)v;
  }
  return V21_OK;
}

int nuis_upload(v21_mlp* m, const NuisRecord& rec) {
  hipStream_t st = m->ctx->stream;
  CHK(m->nu_qf.reserve(rec.qf.size()));
  CHK(m->nu_qd.reserve(rec.q.size()));
  CHK(m->lk_proj.reserve(rec.proj.size()));
  HIPCHK(hipMemcpyAsync(m->nu_qf.p, rec.qf.data(), rec.qf.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(m->nu_qd.p, rec.q.data(), rec.q.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(m->lk_proj.p, rec.proj.data(), rec.proj.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return V21_OK;
}

extern "C" int v21_mlp_set_nuisance(v21_mlp* m, const double* basis, int32_t n_modes, int32_t out_dim) {
  if (!m) return fail(V21_ERR_ARG, "null mlp");
  if (!basis) { m->nu_k = 0; return V21_OK; }
  if (!m->has_lk) return fail(V21_ERR_STATE, "nuisance modes need a likelihood record (v21_mlp_set_likelihood)");
  const int dout = m->dims[m->L];
  if (out_dim != dout) return fail(V21_ERR_ARG, "nuisance: %d bins, stack output = %d", (int)out_dim, dout);
  NuisRecord rec;
  CHK(nuis_build(basis, m->lk_h_w.data(), m->lk_h_data.data(), n_modes, dout, rec));
  CHK(use(m->ctx));
  CHK(nuis_upload(m, rec));
  m->nu_basis.assign(basis, basis + (size_t)n_modes * dout);
  m->nu = std::move(rec);
  m->nu_k = n_modes;
  return V21_OK;
}

extern "C" int v21_mlp_nuisance_info(v21_mlp* m, int32_t* n_modes) {
  if (!m || !n_modes) return fail(V21_ERR_ARG, "null argument");
  *n_modes = m->nu_k;
  return V21_OK;
}

int nuis_project(v21_mlp* m, const float* d_data, long long n_data, const float** out) {
  *out = d_data;
  if (!m->nu_k) return V21_OK;
  const int dout = m->dims[m->L];
  CHK(m->nu_ws.reserve((size_t)n_data * dout));
  hipLaunchKernelGGL(nuis_project_kernel, dim3((unsigned)((n_data + 3) / 4)), dim3(256), 0, m->ctx->stream, d_data, m->lk_w.get(),
                     m->nu_qd.get(), m->nu_k, m->nu_ws.get(), n_data, dout);
  HIPCHK(hipGetLastError());
  *out = m->nu_ws.get();
  return V21_OK;
}

static constexpr JacEntry kCoef{"nuisance amplitudes", kJacMaxIn, true, false};

// a_hat[n, :] = R^-1 (Q W (d_raw - y[n])): the kernel's b is taken against the projected data, Q W d_raw is the record's
extern "C" int v21_mlp_nuisance_coef(v21_mlp* m, const void* x, int x_dtype, int64_t n, double* coef, int precision, int flags) {
  CHK(jac_args(m, x && coef, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kCoef));
  if (!m->nu_k) return fail(V21_ERR_STATE, "nuisance amplitudes requested but no nuisance modes set (v21_mlp_set_nuisance)");
  if (n == 0) return V21_OK;
  const int K = m->nu_k;
  const int route = jac_route(m, precision, flags, m->dims[m->L]);
  std::vector<float> b((size_t)n * K);
  ChunkStage sg;
  float* db;
  sg.add(b.data(), &db, K * sizeof(float));
  CHK(jac_chunks(m, x, x_dtype, n, flags & V21_FWD_IN_TRANSFORM, sg, [&](long long, long long rows) {
    return reduce_run(m, route, rows, nullptr, nullptr, nullptr, db, m->lk_proj.get(), 0, 1, 0, precision, flags);
  }));
  const double* R = m->nu.r.data();
  for (long long i = 0; i < n; ++i)
    for (int j = K - 1; j >= 0; --j) {
      double s = (double)b[(size_t)i * K + j] + m->nu.cd[j];
      for (int l = j + 1; l < K; ++l) s -= R[(size_t)j * K + l] * coef[i * K + l];
      coef[i * K + j] = s / R[(size_t)j * K + j];
    }
  return V21_OK;
}
