// hooks/gbp_debug_vertex.hip — TEST HOOK (include/gbp_mi355x_debug.h: gbp_debug_vertex): the PRODUCT's vertex layer — relin_core and
// factor_update of kernels/gbp_vertex.hpp, the code every sweep kernel runs per lane — on caller-supplied factors, one lane per case, in the
// reference's tensor names and layouts.  Included by gbp_kernels.hip when the library is built with
// -DGBP_BUILD_TEST_HOOKS (libgbp_mi355x_test.so); the product library does not contain it.
//
// A case is one factor's complete vertex input; the lane packs it into the FAC[56] / literal camera message [28] / LMSG[16] / CAMB[44] / LMKB[16] records
// as the upload and the belief kernels lay them out, runs one op and unpacks every output:
//   op 0  RelineariseFactorVertex (gbp_codelets.cpp:20-172) as k_linearise does it: potential zeroed, belief_means, cam_lin, relin_core
//   op 1  PrepMessageVertex + the four Compute*Message*Vertex classes (gbp_codelets.cpp:215-710): factor_update<false> (per-factor means)
//   op 2  the same through factor_update<true>: the means, the dmu^2 pieces and the camera's CAM_LIN record are produced first with the
//         belief owners' own routines (cam_mean / cam_dmu2 / cam_lin + cam_lin_pack, lmk_mean / lmk_dmu2: beliefs_body) and reach the
//         relinearising lane as in sweep_tile (float4 means, cam_lin_unpack, lmk_mean on the record)
// input record, kVtxIn floats (integers as their bit patterns):
//   K 9 | measurement 2 | meas_variance 1 | kf_belief eta 6, lambda 36 | lmk_belief eta 3, lambda 9 | factor eta 9, lambda 81 = [cc36|cl18|lc18|ll9]
//   | previous cam message eta 6, lambda 36 | previous lmk message eta 3, lambda 9 | oldmu 9 | damping 1 | damping_count (int) | active_flag (uint)
//   | robust_flag before (uint) | maxeta_damping, num_undamped_iters (int), dmu_threshold, min_linear_iters (int), nstds, relin_mode (int)
// The packed records hold what the device keeps: the lower triangles of Lambda_cc / Lambda_ll and of the previous camera message,
// Lambda_cl (Lambda_lc is its transpose).
// output record, kVtxOut floats:
//   factor eta 9, lambda 81 | cam message eta 6, lambda 36 (all 36 entries: what goes into the row sums) | lmk message eta 3, lambda 9
//   | mu 9 (op 2: the hoisted means; that mode keeps no per-factor mu) | dmu | damping | damping_count (int) | robust_flag (uint)
//   op 0 writes the potential and the robust flag, zeros elsewhere.
#pragma once
#include "../kernels/gbp_tile.hpp"
#include "../kernels/gbp_vertex.hpp"

namespace gbp {
using namespace gbpdev;

constexpr int kVtxIn = 229, kVtxOut = 157;

template <int OP>
__global__ __launch_bounds__(64) void k_debug_vertex(const float* __restrict__ in, float* __restrict__ out, int n) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const float* x = in + (size_t)t * kVtxIn;
  float* y = out + (size_t)t * kVtxOut;
  constexpr int iK = 0, iZ = 9, iVar = 11, iCbe = 12, iCbl = 18, iLbe = 54, iLbl = 57, iFe = 66, iFl = 75, iPce = 156, iPcl = 162, iPle = 198,
                iPll = 201, iOldmu = 210, iDamp = 219, iCount = 220, iActive = 221, iRobust = 222, iHyper = 223;
  constexpr int oFe = 0, oFl = 9, oMce = 90, oMcl = 96, oMle = 132, oMll = 135, oMu = 144, oDmu = 153, oDamp = 154, oCount = 155, oRobust = 156;

  float fac[56], cm[28], mu[12], lm[16], cb[44], lb[16], K[9];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) K[i] = x[iK + i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) fac[i] = x[iFe + i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) fac[9 + tri(i, j)] = x[iFl + i * 6 + j];
  }
  GBP_UNROLL
  for (int i = 0; i < 18; ++i) fac[30 + i] = x[iFl + 36 + i];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) fac[48 + tri(i, j)] = x[iFl + 72 + i * 3 + j];
  }
  fac[54] = x[iZ]; fac[55] = x[iZ + 1];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) cm[i] = x[iPce + i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) cm[6 + tri(i, j)] = x[iPcl + i * 6 + j];
  }
  cm[27] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 16; ++i) lm[i] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) lm[i] = x[iPle + i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) lm[4 + i] = x[iPll + i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) cb[i] = x[iCbe + i];
  cb[6] = 0.f; cb[7] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 36; ++i) cb[8 + i] = x[iCbl + i];
  GBP_UNROLL
  for (int i = 0; i < 16; ++i) lb[i] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) lb[i] = x[iLbe + i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) lb[4 + i] = x[iLbl + i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) mu[i] = x[iOldmu + i];      // mu == oldmu between sweeps (ba.cpp:898)
  mu[9] = 0.f; mu[10] = 0.f; mu[11] = 0.f;

  Hyper hp;
  hp.maxeta_damping = x[iHyper];
  hp.num_undamped_iters = __float_as_int(x[iHyper + 1]);
  hp.dmu_threshold = x[iHyper + 2];
  hp.min_linear_iters = __float_as_int(x[iHyper + 3]);
  hp.nstds = x[iHyper + 4];
  hp.relin_mode = __float_as_int(x[iHyper + 5]);
  const float var = x[iVar];
  float damping = x[iDamp];
  int count = __float_as_int(x[iCount]);
  const bool active = __float_as_uint(x[iActive]) == 1u;
  uint32_t flags = (active ? kFlagActive : 0u) | (__float_as_uint(x[iRobust]) != 0u ? kFlagRobust : 0u);

  float oc_eta[6], oc_lam[36], bi[9], ol[16], mu_out[9];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) oc_eta[i] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 36; ++i) oc_lam[i] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 16; ++i) ol[i] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) mu_out[i] = 0.f;

  if (OP == 0) {   // k_linearise's body
    float x0c[6], x0l[3];
    GBP_UNROLL
    for (int i = 0; i < 54; ++i) fac[i] = 0.f;
    belief_means(cb, lb, x0c, x0l);
    CamLin cl;
    const float wv[3] = {x0c[3], x0c[4], x0c[5]};
    cam_lin(wv, cl);
    const bool robust = relin_core(fac, x0c, x0l, K, var, hp.nstds, cl);
    flags = robust ? (flags | kFlagRobust) : (flags & ~kFlagRobust);
    damping = 0.f; count = 0;
  } else if (OP == 1) {
    bool relin;
    factor_update<false>(fac, cm, mu, lm, cb, lb, K, hp, damping, count, flags, var, active, oc_eta, oc_lam, bi, ol, relin,
                         [&](float (&)[6], float (&)[3], CamLin&, float&) {});
    GBP_UNROLL
    for (int i = 0; i < 9; ++i) mu_out[i] = mu[i];
  } else {
    // what the belief owners leave for the next sweep (beliefs_body): camera mean, its dmu^2 prefix (belief slot 6) and CAM_LIN record;
    // landmark mean and its three dmu^2 terms (belief slots 3, 13, 14); `used` = the means the last sweep used = oldmu
    float x0c_h[6], x0l_h[3], u[3];
    cam_mean(cb, x0c_h);
    const float used[6] = {mu[0], mu[1], mu[2], mu[3], mu[4], mu[5]};
    const float S = cam_dmu2(used, x0c_h);
    const float4 m0 = make_float4(x0c_h[0], x0c_h[1], x0c_h[2], x0c_h[3]), m1 = make_float4(x0c_h[4], x0c_h[5], 0.f, 0.f);
    float4 q[kCamLin4];
    {
      CamLin clh;
      const float wv[3] = {x0c_h[3], x0c_h[4], x0c_h[5]};
      cam_lin(wv, clh);
      cam_lin_pack(clh, q);
    }
    lmk_mean(lb, x0l_h);
    lmk_dmu2(make_float4(mu[6], mu[7], mu[8], 0.f), x0l_h, u);
    cb[6] = S;
    lb[3] = u[0]; lb[13] = u[1]; lb[14] = u[2];
    bool relin;
    factor_update<true>(fac, cm, mu, lm, cb, lb, K, hp, damping, count, flags, var, active, oc_eta, oc_lam, bi, ol, relin,
                        [&](float (&x0c)[6], float (&x0l)[3], CamLin& cl, float&) {      // as sweep_tile hands them to a relinearising lane
                          x0c[0] = m0.x; x0c[1] = m0.y; x0c[2] = m0.z; x0c[3] = m0.w; x0c[4] = m1.x; x0c[5] = m1.y;
                          cam_lin_unpack(q, cl);
                          lmk_mean(lb, x0l);
                        });
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) mu_out[i] = x0c_h[i];
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) mu_out[6 + i] = x0l_h[i];
  }

  GBP_UNROLL
  for (int i = 0; i < 9; ++i) y[oFe + i] = fac[i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 6; ++j) y[oFl + i * 6 + j] = fac[9 + trisym(i, j)];
  }
  GBP_UNROLL
  for (int i = 0; i < 18; ++i) y[oFl + 36 + i] = fac[30 + i];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 6; ++j) y[oFl + 54 + i * 6 + j] = fac[30 + j * 3 + i];      // Lambda_lc = Lambda_cl^T
  }
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 3; ++j) y[oFl + 72 + i * 3 + j] = fac[48 + trisym(i, j)];
  }
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) y[oMce + i] = oc_eta[i];
  GBP_UNROLL
  for (int i = 0; i < 36; ++i) y[oMcl + i] = oc_lam[i];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) y[oMle + i] = ol[i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) y[oMll + i] = ol[4 + i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) y[oMu + i] = mu_out[i];
  y[oDmu] = mu[9];
  y[oDamp] = damping;
  y[oCount] = __int_as_float(count);
  y[oRobust] = __uint_as_float((flags & kFlagRobust) != 0u ? 1u : 0u);
}

// gbp_debug_get(what = 1): the camera messages as the reference stores them, from the CMSG records — cmsg_expand, as every sweep
// runs it; out[p] = eta 6, Lambda lower triangle 21, 0
__global__ __launch_bounds__(256) void k_cmsg_expand(const SweepArgs a, float* __restrict__ out) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x, tile = p >> 6, lane = p & 63;
  float fac[56], rec[16], cm[28];
  load_tile<kFacG, false>(a.fac, tile, lane, fac);
  load_tile<kCmsgG, false>(a.cmsg, tile, lane, rec);
  cmsg_expand(fac, rec, a.cmsg_lit, tile, lane, cm);
  GBP_UNROLL
  for (int i = 0; i < 28; ++i) out[(size_t)p * 28 + i] = cm[i];
}
void launch_cmsg_expand(const SweepArgs& a, uint32_t n_tiles, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_cmsg_expand, dim3(n_tiles / 4), dim3(256), 0, s, a, out);
}

// reached through debug_math_widths / launch_debug_math (hooks/gbp_debug_math.hip) as ops kDebugVertexOp0 + op
static bool debug_vertex_widths(int op, int* in_w, int* out_w) {
  if (op < 0 || op > 2) return false;
  *in_w = kVtxIn; *out_w = kVtxOut;
  return true;
}
static void launch_debug_vertex(int op, const float* in, float* out, int n, hipStream_t s) {
  if (op < 0 || op > 2 || n <= 0) return;
  const dim3 grid((n + 63) / 64), block(64);
  if (op == 0) hipLaunchKernelGGL(k_debug_vertex<0>, grid, block, 0, s, in, out, n);
  else if (op == 1) hipLaunchKernelGGL(k_debug_vertex<1>, grid, block, 0, s, in, out, n);
  else hipLaunchKernelGGL(k_debug_vertex<2>, grid, block, 0, s, in, out, n);
}

}  // namespace gbp
