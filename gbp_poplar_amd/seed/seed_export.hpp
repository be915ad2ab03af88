// seed/seed_export.hpp — how a function of include/gbp_mi355x_seed.h is defined: the guard of csrc/gbp_export.hpp for a library
// without a ctx.  The text of a failure goes to the calling thread (gbp_seed_last_error).
#pragma once
#include "../../include/gbp_mi355x_seed.h"

#include <exception>
#include <new>
#include <string>

namespace gbp {
namespace seed {

inline std::string& last_error() {
  thread_local std::string g_error;
  return g_error;
}
inline int fail(int code, const std::string& msg) {
  last_error() = msg;
  return code;
}

// No C++ exception crosses the C-ABI: every exported function runs its body inside this guard.
template <class F> int guarded(const char* what, F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(GBP_ERR_NOMEM, std::string(what) + ": out of host memory");
  } catch (const std::exception& e) {
    return fail(GBP_ERR_INVALID, std::string(what) + ": " + e.what());
  } catch (...) {
    return fail(GBP_ERR_INVALID, std::string(what) + ": unknown exception");
  }
}

// EVERY function the header declares is DEFINED through one of these two macros: the exported symbol is a shell around
// `<name>_body`, which the macro leaves open for the function's body (tests/test_seed_cpu.py greps seed/ for an export defined any
// other way).
#define GBP_SEED_EXPORT(name, sig, call)                                                                                \
  static int name##_body sig;                                                                                           \
  extern "C" GBP_API int name sig { return ::gbp::seed::guarded(#name, [&]() -> int { return name##_body call; }); }    \
  static int name##_body sig
#define GBP_SEED_EXPORT_T(ret, fallback, name, sig, call)                                                 \
  static ret name##_body sig;                                                                             \
  extern "C" GBP_API ret name sig { try { return name##_body call; } catch (...) { return fallback; } }   \
  static ret name##_body sig

}  // namespace seed
}  // namespace gbp
