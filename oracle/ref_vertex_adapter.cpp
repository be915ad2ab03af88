// ref_vertex_adapter.cpp — TEST INFRASTRUCTURE ONLY, built in the build container only (`make -C oracle ref`).
//
// The REFERENCE's seven vertex classes (ba/gbp_codelets.cpp) behind a C interface, one function per class.  The file is
// #included where it lies under $(REF)/ba (the Makefile passes -I$(REF)/ba; no copy is made into this repository, the objects
// go to $(REFOUT), outside it) and compiled UNMODIFIED against poplar_standin/poplar/Vertex.hpp, our stand-in for the field
// wrappers (Input / Output / InOut / Vector): each rv_* function points the fields of a vertex object at the caller's arrays
// and runs the reference's own compute() body.  Arguments carry the reference's field names; the message vertices' *_dofs
// fields are the fixed 6 (camera) / 3 (landmark) of ba.cpp.  What this does not pin: the graph wiring of ba.cpp and the
// summation order of popops::reduceWithOutput.
#include <cmath>
#include <type_traits>
#include <utility>
#include "gbp_codelets.cpp"

// The expressions the arithmetic depends on have the types Poplar's wrappers would give them.
static_assert(std::is_same<decltype(*std::declval<PrepMessageVertex&>().damping), float&>::value, "*damping is the float itself");
static_assert(std::is_same<decltype(*std::declval<PrepMessageVertex&>().damping_count), int&>::value, "*damping_count is the int itself");
static_assert(std::is_same<decltype(std::sqrt(std::declval<PrepMessageVertex&>().meas_variance)), float>::value,
              "std::sqrt(Input<float>) is the float overload");
static_assert(std::is_same<decltype(std::sqrt(std::declval<PrepMessageVertex&>().dmu)), float>::value,
              "std::sqrt(InOut<float>) is the float overload");
static_assert(std::is_same<decltype(Nstds * std::sqrt(std::declval<PrepMessageVertex&>().meas_variance)), float>::value,
              "the Huber threshold is a float expression");
static_assert(std::is_same<decltype(0.5 * Nstds * Nstds * std::declval<PrepMessageVertex&>().meas_variance), double>::value,
              "the 0.5 literal makes the Huber denominator a double expression");
static_assert(std::is_same<decltype(1 - std::declval<ComputeCamMessageEtaVertex&>().damping), float>::value, "1 - damping is a float");
static_assert(std::is_same<decltype(std::declval<WeakenPriorVertex&>().weaken_flag - 5), unsigned>::value,
              "weaken_flag meets an int literal as unsigned (the conversions of `weaken_flag == 5`)");
static_assert(std::is_same<decltype(std::declval<PrepMessageVertex&>().active_flag - 1), unsigned>::value,
              "active_flag meets an int literal as unsigned");
static_assert(std::is_same<decltype(*std::declval<PrepMessageVertex&>().damping_count > min_linear_iters - num_undamped_iters), bool>::value &&
              std::is_same<decltype(min_linear_iters - num_undamped_iters), int>::value, "the relinearisation count test is an int comparison");

namespace {
float* nc(const float* p) { return const_cast<float*>(p); }

template <class V>
void bind_potential(V& v, float* factor_eta, float* cc, float* ll, float* cl, float* lc) {
  v.factor_eta_.bind(factor_eta, 9);
  v.factor_lambda_cc_.bind(cc, 36);
  v.factor_lambda_ll_.bind(ll, 9);
  v.factor_lambda_cl_.bind(cl, 18);
  v.factor_lambda_lc_.bind(lc, 18);
}
template <class V>
void bind_beliefs(V& v, const float* measurement, const float* meas_variance, const float* K, const float* kf_eta, const float* kf_lambda,
                  const float* lmk_eta, const float* lmk_lambda) {
  v.measurement.bind(nc(measurement), 2);
  v.meas_variance.bind(nc(meas_variance));
  v.K_.bind(nc(K), 9);
  v.kf_belief_eta_.bind(nc(kf_eta), 6);
  v.kf_belief_lambda_.bind(nc(kf_lambda), 36);
  v.lmk_belief_eta_.bind(nc(lmk_eta), 3);
  v.lmk_belief_lambda_.bind(nc(lmk_lambda), 9);
}
// the message vertices: oe = the variable the message goes to, noe = the other one
template <class V>
void bind_eta(V& v, unsigned oe, unsigned noe, const float* damping, const unsigned* active_flag, const unsigned* oe_dofs, const unsigned* noe_dofs,
              const float* f_outedge_eta, const float* f_nonoutedge_eta, const float* f_noe_noe_lambda, const float* f_oe_noe_lambda,
              const float* belief_nonoutedge_eta, const float* belief_nonoutedge_lambda, const float* pmess_nonoutedge_eta,
              const float* pmess_nonoutedge_lambda, const float* pmess_outedge_eta, float* mess_outedge_eta) {
  v.damping.bind(nc(damping));
  v.active_flag.bind(const_cast<unsigned*>(active_flag));
  v.outedge_dofs.bind(const_cast<unsigned*>(oe_dofs));
  v.nonoutedge_dofs.bind(const_cast<unsigned*>(noe_dofs));
  v.f_outedge_eta_.bind(nc(f_outedge_eta), oe);
  v.f_nonoutedge_eta_.bind(nc(f_nonoutedge_eta), noe);
  v.f_noe_noe_lambda_.bind(nc(f_noe_noe_lambda), noe * noe);
  v.f_oe_noe_lambda_.bind(nc(f_oe_noe_lambda), oe * noe);
  v.belief_nonoutedge_eta_.bind(nc(belief_nonoutedge_eta), noe);
  v.belief_nonoutedge_lambda_.bind(nc(belief_nonoutedge_lambda), noe * noe);
  v.pmess_nonoutedge_eta_.bind(nc(pmess_nonoutedge_eta), noe);
  v.pmess_nonoutedge_lambda_.bind(nc(pmess_nonoutedge_lambda), noe * noe);
  v.pmess_outedge_eta_.bind(nc(pmess_outedge_eta), oe);
  v.mess_outedge_eta_.bind(mess_outedge_eta, oe);
}
template <class V>
void bind_lambda(V& v, unsigned oe, unsigned noe, const unsigned* active_flag, const unsigned* oe_dofs, const unsigned* noe_dofs,
                 const float* f_oe_oe_lambda, const float* f_noe_noe_lambda, const float* f_oe_noe_lambda, const float* f_noe_oe_lambda,
                 const float* belief_nonoutedge_lambda, const float* pmess_nonoutedge_lambda, float* mess_outedge_lambda) {
  v.active_flag.bind(const_cast<unsigned*>(active_flag));
  v.outedge_dofs.bind(const_cast<unsigned*>(oe_dofs));
  v.nonoutedge_dofs.bind(const_cast<unsigned*>(noe_dofs));
  v.f_oe_oe_lambda_.bind(nc(f_oe_oe_lambda), oe * oe);
  v.f_noe_noe_lambda_.bind(nc(f_noe_noe_lambda), noe * noe);
  v.f_oe_noe_lambda_.bind(nc(f_oe_noe_lambda), oe * noe);
  v.f_noe_oe_lambda_.bind(nc(f_noe_oe_lambda), noe * oe);
  v.belief_nonoutedge_lambda_.bind(nc(belief_nonoutedge_lambda), noe * noe);
  v.pmess_nonoutedge_lambda_.bind(nc(pmess_nonoutedge_lambda), noe * noe);
  v.mess_outedge_lambda_.bind(mess_outedge_lambda, oe * oe);
}
const unsigned kCamDofs = 6, kLmkDofs = 3;
}  // namespace

extern "C" {

const char* rv_impl_name(void) { return "reference"; }

// the globals of gbp_codelets.cpp:11-16
void rv_set_hyper(float maxeta_damping_, int num_undamped_iters_, float dmu_threshold_, int min_linear_iters_, float nstds_) {
  maxeta_damping = maxeta_damping_;
  num_undamped_iters = num_undamped_iters_;
  dmu_threshold = dmu_threshold_;
  min_linear_iters = min_linear_iters_;
  Nstds = nstds_;
}

void rv_relinearise_factor(const float* measurement, float meas_variance, const float* K, const float* kf_belief_eta,
                           const float* kf_belief_lambda, const float* lmk_belief_eta, const float* lmk_belief_lambda, float* factor_eta,
                           float* factor_lambda_cc, float* factor_lambda_ll, float* factor_lambda_cl, float* factor_lambda_lc,
                           unsigned* robust_flag) {
  RelineariseFactorVertex v;
  bind_beliefs(v, measurement, &meas_variance, K, kf_belief_eta, kf_belief_lambda, lmk_belief_eta, lmk_belief_lambda);
  bind_potential(v, factor_eta, factor_lambda_cc, factor_lambda_ll, factor_lambda_cl, factor_lambda_lc);
  v.robust_flag.bind(robust_flag);
  v.compute();
}

void rv_prep_message(float* damping, int* damping_count, unsigned active_flag, unsigned* robust_flag, const float* measurement, const float* K,
                     float meas_variance, const float* kf_belief_eta, const float* kf_belief_lambda, const float* lmk_belief_eta,
                     const float* lmk_belief_lambda, const float* oldmu, float* mu, float* dmu, float* factor_eta, float* factor_lambda_cc,
                     float* factor_lambda_ll, float* factor_lambda_cl, float* factor_lambda_lc) {
  PrepMessageVertex v;
  v.damping.bind(damping);
  v.damping_count.bind(damping_count);
  v.active_flag.bind(&active_flag);
  v.robust_flag.bind(robust_flag);
  bind_beliefs(v, measurement, &meas_variance, K, kf_belief_eta, kf_belief_lambda, lmk_belief_eta, lmk_belief_lambda);
  v.oldmu.bind(nc(oldmu), 9);
  v.mu.bind(mu, 9);
  v.dmu.bind(dmu);
  bind_potential(v, factor_eta, factor_lambda_cc, factor_lambda_ll, factor_lambda_cl, factor_lambda_lc);
  v.compute();
}

void rv_cam_message_eta(float damping, unsigned active_flag, const float* f_outedge_eta, const float* f_nonoutedge_eta,
                        const float* f_noe_noe_lambda, const float* f_oe_noe_lambda, const float* belief_nonoutedge_eta,
                        const float* belief_nonoutedge_lambda, const float* pmess_nonoutedge_eta, const float* pmess_nonoutedge_lambda,
                        const float* pmess_outedge_eta, float* mess_outedge_eta) {
  ComputeCamMessageEtaVertex v;
  bind_eta(v, kCamDofs, kLmkDofs, &damping, &active_flag, &kCamDofs, &kLmkDofs, f_outedge_eta, f_nonoutedge_eta, f_noe_noe_lambda,
           f_oe_noe_lambda, belief_nonoutedge_eta, belief_nonoutedge_lambda, pmess_nonoutedge_eta, pmess_nonoutedge_lambda, pmess_outedge_eta,
           mess_outedge_eta);
  v.compute();
}

void rv_lmk_message_eta(float damping, unsigned active_flag, const float* f_outedge_eta, const float* f_nonoutedge_eta,
                        const float* f_noe_noe_lambda, const float* f_oe_noe_lambda, const float* belief_nonoutedge_eta,
                        const float* belief_nonoutedge_lambda, const float* pmess_nonoutedge_eta, const float* pmess_nonoutedge_lambda,
                        const float* pmess_outedge_eta, float* mess_outedge_eta) {
  ComputeLmkMessageEtaVertex v;
  bind_eta(v, kLmkDofs, kCamDofs, &damping, &active_flag, &kLmkDofs, &kCamDofs, f_outedge_eta, f_nonoutedge_eta, f_noe_noe_lambda,
           f_oe_noe_lambda, belief_nonoutedge_eta, belief_nonoutedge_lambda, pmess_nonoutedge_eta, pmess_nonoutedge_lambda, pmess_outedge_eta,
           mess_outedge_eta);
  v.compute();
}

void rv_cam_message_lambda(unsigned active_flag, const float* f_oe_oe_lambda, const float* f_noe_noe_lambda, const float* f_oe_noe_lambda,
                           const float* f_noe_oe_lambda, const float* belief_nonoutedge_lambda, const float* pmess_nonoutedge_lambda,
                           float* mess_outedge_lambda) {
  ComputeCamMessageLambdaVertex v;
  bind_lambda(v, kCamDofs, kLmkDofs, &active_flag, &kCamDofs, &kLmkDofs, f_oe_oe_lambda, f_noe_noe_lambda, f_oe_noe_lambda, f_noe_oe_lambda,
              belief_nonoutedge_lambda, pmess_nonoutedge_lambda, mess_outedge_lambda);
  v.compute();
}

void rv_lmk_message_lambda(unsigned active_flag, const float* f_oe_oe_lambda, const float* f_noe_noe_lambda, const float* f_oe_noe_lambda,
                           const float* f_noe_oe_lambda, const float* belief_nonoutedge_lambda, const float* pmess_nonoutedge_lambda,
                           float* mess_outedge_lambda) {
  ComputeLmkMessageLambdaVertex v;
  bind_lambda(v, kLmkDofs, kCamDofs, &active_flag, &kLmkDofs, &kCamDofs, f_oe_oe_lambda, f_noe_noe_lambda, f_oe_noe_lambda, f_noe_oe_lambda,
              belief_nonoutedge_lambda, pmess_nonoutedge_lambda, mess_outedge_lambda);
  v.compute();
}

void rv_weaken_prior(float scaling, unsigned* weaken_flag, float* prior_eta, unsigned n_eta, float* prior_lambda, unsigned n_lambda) {
  WeakenPriorVertex v;
  v.scaling.bind(&scaling);
  v.weaken_flag.bind(weaken_flag);
  v.prior_eta.bind(prior_eta, n_eta);
  v.prior_lambda.bind(prior_lambda, n_lambda);
  v.compute();
}

}  // extern "C"
