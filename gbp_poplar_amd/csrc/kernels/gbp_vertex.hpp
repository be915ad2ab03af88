// kernels/gbp_vertex.hpp — the vertex layer: the reference's compute() bodies (gbp_codelets.cpp, bafuncs.cpp) on register
// records, one lane per factor or per variable.  Device helpers only; k_sweep, k_linearise, the belief owners and the persistent
// kernels all run THESE copies, so every path produces the same bits.
#pragma once
#include "gbp_tile.hpp"      // load_tile (cmsg_expand: the literal camera messages)

namespace gbp {
using namespace gbpdev;

// The arithmetic of a belief owner, shared by every kernel that updates beliefs (k_beliefs, both persistent kernels) and by the
// sweep that recomputes a landmark mean: one copy of the operations, so every path produces the same bits.
// inf2mean3x3 (bafuncs.cpp:11-15) on a 16-float landmark record (eta at 0..2, Lambda at 4..12)
GBP_DEV void lmk_mean(const float (&rec)[16], float (&x0l)[3]) {
  float B[9], S3[9];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) B[i] = rec[4 + i];
  inv3x3(B, S3);
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    float acc = 0.f;
    GBP_UNROLL
    for (int k = 0; k < 3; ++k) acc += S3[i * 3 + k] * rec[k];
    x0l[i] = acc;
  }
}
// mean of a camera belief record (44 floats, in registers or in LDS): inf2mean6x6 (bafuncs.cpp:2-9)
template <class REC>
GBP_DEV void cam_mean(REC&& cb, float (&x0c)[6]) {
  solve6_lower([&](int i, int j) { return cb[8 + i * 6 + j]; }, [&](int k) { return cb[k]; }, x0c);
}
// the dmu^2 pieces of the next sweep (k_sweep<HOIST>): the camera prefix S (belief slot 6) and the three landmark terms (slots 3, 13, 14)
GBP_DEV float cam_dmu2(const float (&used)[6], const float (&x0c)[6]) {
  float S = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) S += (used[i] - x0c[i]) * (used[i] - x0c[i]);
  return S;
}
GBP_DEV void lmk_dmu2(const float4 used, const float (&x0l)[3], float (&u)[3]) {
  u[0] = (used.x - x0l[0]) * (used.x - x0l[0]);
  u[1] = (used.y - x0l[1]) * (used.y - x0l[1]);
  u[2] = (used.z - x0l[2]) * (used.z - x0l[2]);
}

// belief means: inf2mean6x6 / inf2mean3x3 (bafuncs.cpp:2-15) on CAMB / LMKB records
GBP_DEV void belief_means(const float (&cb)[44], const float (&lb)[16], float (&x0c)[6], float (&x0l)[3]) {
  float Al[21], S6[36];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) Al[tri(i, j)] = cb[8 + i * 6 + j];
  }
  inv6x6_lower(Al, S6);
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    float acc = 0.f;
    GBP_UNROLL
    for (int k = 0; k < 6; ++k) acc += S6[i * 6 + k] * cb[k];
    x0c[i] = acc;
  }
  lmk_mean(lb, x0l);
}

// Shared body of gbp_codelets.cpp:90-168 and :294-373 on the packed FAC record: accumulate
// J^T J / J^T (J x0 + z - h(x0)) onto the potential, Huber-rescale.  Returns the robust flag.
GBP_DEV bool relin_core(float (&fac)[56], const float (&x0c)[6], const float (&x0l)[3], const float (&K)[9],
                        float var, float nstds, const CamLin& cl /* == cam_lin(x0c[3..5]) */) {
  Lin L;
  jac_hfunc_lin(x0c, x0l, K, cl, L);
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) {
      float acc = fac[9 + tri(i, j)];
      GBP_UNROLL
      for (int k = 0; k < 2; ++k) acc += L.Jkf[k * 6 + i] * L.Jkf[k * 6 + j];
      fac[9 + tri(i, j)] = acc;
    }
  }
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) {
      float acc = fac[48 + tri(i, j)];
      GBP_UNROLL
      for (int k = 0; k < 2; ++k) acc += L.Jl[k * 3 + i] * L.Jl[k * 3 + j];
      fac[48 + tri(i, j)] = acc;
    }
  }
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 3; ++j) {
      float acc = fac[30 + i * 3 + j];
      GBP_UNROLL
      for (int k = 0; k < 2; ++k) acc += L.Jkf[k * 6 + i] * L.Jl[k * 3 + j];
      fac[30 + i * 3 + j] = acc;
    }
  }
  const float z0 = fac[54], z1 = fac[55];
  float buf[2];
  GBP_UNROLL
  for (int r = 0; r < 2; ++r) {
    float acc = 0.f;
    GBP_UNROLL
    for (int k = 0; k < 6; ++k) acc += L.Jkf[r * 6 + k] * x0c[k];
    GBP_UNROLL
    for (int k = 0; k < 3; ++k) acc += L.Jl[r * 3 + k] * x0l[k];
    acc = acc + (r == 0 ? z0 : z1);
    acc = acc - L.hx[r];
    buf[r] = acc;
  }
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) {
    float acc = fac[i];
    GBP_UNROLL
    for (int k = 0; k < 2; ++k) acc += (i < 6 ? L.Jkf[k * 6 + i] : L.Jl[k * 3 + (i - 6)]) * buf[k];
    fac[i] = acc;
  }
  // Huber (gbp_codelets.cpp:135-141): the 0.5 literal makes the denominator a double expression
  const float err = sqrtf((L.hx[0] - z0) * (L.hx[0] - z0) + (L.hx[1] - z1) * (L.hx[1] - z1));
  float mvar = var;
  const bool robust = err > nstds * sqrtf(var);
  if (robust) {
    const double den = 2 * ((double)(nstds * sqrtf(var) * err) - 0.5 * (double)nstds * (double)nstds * (double)var);
    mvar = (float)((double)(var * err * err) / den);
  }
  {  // 54 divisions by one divisor (gbp_codelets.cpp:142-168, 343-373): exact through one fp64 reciprocal
    float num[54], quo[54];
    GBP_UNROLL
    for (int i = 0; i < 54; ++i) num[i] = fac[i];
    div_shared(num, mvar, quo);
    GBP_UNROLL
    for (int i = 0; i < 54; ++i) fac[i] = quo[i];
  }
  return robust;
}

// The Lambda half of ComputeCamMessage{Eta,Lambda}Vertex (gbp_codelets.cpp:411-471, 592-637) from the potential and the 3x3 inverse Bi:
// G2 = Lambda_cl Bi, then put(i, j, Lambda_cc(i,j) - sum_k G2(i,k) Lambda_lc(k,j)) — all 36 entries, or (LOWER) the 21 with i >= j.
// THE one copy of these loops: factor_update produces a factor's new message with it, cmsg_expand re-derives the message a CMSG
// record stands for.  Every entry is its own chain (t = 0.f, k = 0, 1, 2), so the same fac and Bi give the same bits wherever it runs.
template <bool LOWER, class Put>
GBP_DEV void cam_msg_lambda(const float (&fac)[56], const float (&Bi)[9], float (&G2)[18], Put&& put) {
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 3; ++j) {
      float acc = 0.f;
      GBP_UNROLL
      for (int k = 0; k < 3; ++k) acc += fac[30 + i * 3 + k] * Bi[k * 3 + j];
      G2[i * 3 + j] = acc;
    }
  }
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j < (LOWER ? i + 1 : 6); ++j) {
      float t = 0.f;
      GBP_UNROLL
      for (int k = 0; k < 3; ++k) t += G2[i * 3 + k] * fac[30 + j * 3 + k];  // Lambda_lc(k,j) = Lambda_cl(j,k)
      put(i, j, fac[9 + trisym(i, j)] - t);
    }
  }
}
// The camera message a factor starts a sweep from — the 28 floats factor_update reads: eta 6, Lambda lower triangle 21, a spare slot —
// out of its CMSG record (gbp_kernels.h) and its potential AS LOADED: the potential that produced the message, so this runs before
// factor_update may relinearise it.  Every lane derives (no branch; a select keeps the zero message of a kCmsgZero record, whose
// potential may hold anything); only kCmsgLiteral lanes — behind a gbp_linearise under live messages, until their next store —
// take the divergent branch to the side array.
GBP_DEV void cmsg_expand(const float (&fac)[56], const float (&rec)[16], const float4* lit, uint32_t tile, uint32_t lane, float (&cm)[28]) {
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) cm[i] = rec[i];
  float Bi[9], G2[18];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) Bi[i] = rec[6 + i];
  const bool derived = rec[15] == kCmsgDerived;
  cam_msg_lambda<true>(fac, Bi, G2, [&](int i, int j, float v) { cm[6 + tri(i, j)] = derived ? v : 0.f; });
  cm[27] = 0.f;
  if (rec[15] == kCmsgLiteral) {
    float l[kCmsgLitG * 4];
    load_tile<kCmsgLitG, false>(lit, tile, lane, l);
    GBP_UNROLL
    for (int i = 0; i < 21; ++i) cm[6 + i] = l[i];
  }
}
// ... and the record an active factor leaves behind (an inactive or pad factor: the zero record)
GBP_DEV void cmsg_pack(const float (&oc_eta)[6], const float (&bi)[9], bool active, float (&rec)[16]) {
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) rec[i] = active ? oc_eta[i] : 0.f;
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) rec[6 + i] = active ? bi[i] : 0.f;
  rec[15] = active ? kCmsgDerived : kCmsgZero;
}

// One factor's share of a sweep on register state: PrepMessageVertex + the four Compute*Message*Vertex classes
// (gbp_codelets.cpp:215-710).  Shared by k_sweep (state streamed from HBM every launch) and k_persist (state kept in
// registers across iterations).  `means(x0c, x0l, cl, var)` supplies the hoisted linearisation point and the camera-only Jacobian
// terms of that point when a lane relinearises, and may replace `var` (a caller that fetches the variance only then).  cm: the previous camera message (cmsg_expand); bi: the 3x3 inverse the new one was
// computed from (written for an active factor only) — with oc_eta what cmsg_pack keeps of it.
template <bool HOIST, class Means>
GBP_DEV void factor_update(float (&fac)[56], const float (&cm)[28], float (&mu)[12], const float (&lm)[16], const float (&cb)[44],
                           const float (&lb)[16], const float (&K)[9], const Hyper& hp, float& damping, int& count, uint32_t& flags,
                           const float var, const bool active, float (&oc_eta)[6], float (&oc_lam)[36], float (&bi)[9], float (&ol)[16],
                           bool& relin, Means&& means) {
  relin = false;
  // (zero messages of an inactive factor are written in the ELSE branch at the bottom: 58 v_mov the wavefronts of a graph
  // with every factor active never execute, instead of an initialisation in front of the branch that all of them do)
  if (active) {
    ol[3] = 0.f; ol[13] = 0.f; ol[14] = 0.f; ol[15] = 0.f;      // (3, 13, 14: the caller's per-factor scalars)
    // ---- PrepMessageVertex, gbp_codelets.cpp:241-378 ----
    if (0 == count) damping = hp.maxeta_damping;
    count += 1;
    float x0c[6], x0l[3];
    CamLin cl;
    float d2;
    float var_r = var;
    if (HOIST) {
      d2 = cb[6];
      d2 += lb[3];
      d2 += lb[13];
      d2 += lb[14];
    } else {
      belief_means(cb, lb, x0c, x0l);
      d2 = 0.f;
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) {
        d2 += (mu[i] - x0c[i]) * (mu[i] - x0c[i]);
        mu[i] = x0c[i];
      }
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        d2 += (mu[6 + i] - x0l[i]) * (mu[6 + i] - x0l[i]);
        mu[6 + i] = x0l[i];
      }
    }
    const float dmu = sqrtf(d2);
    mu[9] = dmu;
    relin = (dmu < hp.dmu_threshold) && (count > hp.min_linear_iters - hp.num_undamped_iters);
    if (relin) {
      // HOIST: linearisation point = the hoisted means + the camera's CAM_LIN record (rare path: loaded only here); either mode: the
      // callback may fetch the variance here
      means(x0c, x0l, cl, var_r);
      if (!HOIST) {
        const float w[3] = {x0c[3], x0c[4], x0c[5]};
        cam_lin(w, cl);
      }
      damping = 0.f;
      count = -hp.num_undamped_iters;
      if (hp.relin_mode == 1) {
        GBP_UNROLL
        for (int i = 0; i < 54; ++i) fac[i] = 0.f;
      }
      const bool robust = relin_core(fac, x0c, x0l, K, var_r, hp.nstds, cl);
      flags = robust ? (flags | kFlagRobust) : (flags & ~kFlagRobust);
    }

    const float omd = 1 - damping;

    // ---- Compute{Lmk}Message{Eta,Lambda}Vertex, gbp_codelets.cpp:503-562, 664-709 ----
    {
      float Ap[21], Ainv[36], G[18], ed[6];
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) {
        GBP_UNROLL
        for (int j = 0; j <= i; ++j) {
          float t = fac[9 + tri(i, j)] + cb[8 + i * 6 + j];
          t = t - cm[6 + tri(i, j)];
          GBP_SLP_FENCE(t);
          Ap[tri(i, j)] = t;
        }
      }
      inv6x6_lower(Ap, Ainv);
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        GBP_UNROLL
        for (int j = 0; j < 6; ++j) {
          float acc = 0.f;
          GBP_UNROLL
          for (int k = 0; k < 6; ++k) acc += fac[30 + k * 3 + i] * Ainv[k * 6 + j];  // Lambda_lc(i,k) = Lambda_cl(k,i)
          G[i * 6 + j] = acc;
        }
      }
      GBP_UNROLL
      for (int k = 0; k < 6; ++k) {
        float t = fac[k] + cb[k];
        t = t - cm[k];
        ed[k] = t;
      }
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        float s = 0.f;
        GBP_UNROLL
        for (int k = 0; k < 6; ++k) s += G[i * 6 + k] * ed[k];
        const float h = fac[6 + i] - s;
        ol[i] = h * omd + lm[i] * damping;
      }
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        GBP_UNROLL
        for (int j = 0; j < 3; ++j) {
          float t = 0.f;
          GBP_UNROLL
          for (int k = 0; k < 6; ++k) t += G[i * 6 + k] * fac[30 + k * 3 + j];
          ol[4 + i * 3 + j] = fac[48 + trisym(i, j)] - t;
        }
      }
    }
    // ---- Compute{Cam}Message{Eta,Lambda}Vertex, gbp_codelets.cpp:411-471, 592-637 ----
    {
      float Bp[9], G2[18], el[3];
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        GBP_UNROLL
        for (int j = 0; j < 3; ++j) {
          float t = fac[48 + trisym(i, j)] + lb[4 + i * 3 + j];
          t = t - lm[4 + i * 3 + j];
          Bp[i * 3 + j] = t;
        }
      }
      inv3x3(Bp, bi);
      cam_msg_lambda<false>(fac, bi, G2, [&](int i, int j, float v) { oc_lam[i * 6 + j] = v; });
      GBP_UNROLL
      for (int k = 0; k < 3; ++k) {
        float t = fac[6 + k] + lb[k];
        t = t - lm[k];
        el[k] = t;
      }
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) {
        float s = 0.f;
        GBP_UNROLL
        for (int k = 0; k < 3; ++k) s += G2[i * 3 + k] * el[k];
        const float h = fac[i] - s;
        oc_eta[i] = h * omd + cm[i] * damping;
      }
    }
  } else {
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) oc_eta[i] = 0.f;
    GBP_UNROLL
    for (int i = 0; i < 36; ++i) oc_lam[i] = 0.f;
    GBP_UNROLL
    for (int i = 0; i < 16; ++i) ol[i] = 0.f;
  }
}

}  // namespace gbp
