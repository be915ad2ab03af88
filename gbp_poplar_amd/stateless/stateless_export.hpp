// stateless/stateless_export.hpp — how a function of a library WITHOUT a ctx (post/, seed/, resect/, locate/) is defined: the guard of
// csrc/gbp_export.hpp with the text of a failure kept per calling thread (gbp_<lib>_last_error), and what every such library's argument
// checks and launches say the same way.  Include it behind the library's public header (GBP_API, the GBP_ERR_* codes) in a HIP
// translation unit.  Not under csrc/: the core library does not depend on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <exception>
#include <new>
#include <string>

namespace gbp {
namespace stateless {

// ONE TEXT PER LIBRARY, per thread: the libraries are built with -fvisibility=hidden and a version script, so this inline function and
// its function-local thread_local are local symbols of each shared object that includes the header.  A process that loads several of
// them never sees one library's failure in another's text (tests/test_stateless_cpu.py pins it).
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

// EVERY function a public header declares is DEFINED through one of these two macros: the exported symbol is a shell around
// `<name>_body`, which the macro leaves open for the function's body (tests/stateless_cabi.py greps the library's directory for an
// export defined any other way).
#define GBP_STATELESS_EXPORT(name, sig, call)                                                                                \
  static int name##_body sig;                                                                                                \
  extern "C" GBP_API int name sig { return ::gbp::stateless::guarded(#name, [&]() -> int { return name##_body call; }); }    \
  static int name##_body sig
#define GBP_STATELESS_EXPORT_T(ret, fallback, name, sig, call)                                            \
  static ret name##_body sig;                                                                             \
  extern "C" GBP_API ret name sig { try { return name##_body call; } catch (...) { return fallback; } }   \
  static ret name##_body sig

// after a launch: GBP_OK, or GBP_ERR_HIP with the runtime's text
inline int launched(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(GBP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err));
  return GBP_OK;
}
inline int null_arg(const char* fn, const char* arg) { return fail(GBP_ERR_INVALID, std::string(fn) + ": " + arg + " is NULL"); }
inline int bad_arg(const char* fn, const std::string& what) { return fail(GBP_ERR_INVALID, std::string(fn) + ": " + what); }
// an option (name: "opts.<field>") that has to be a positive number / must not be NaN: GBP_OK, or the failure
inline int need_positive(const char* fn, const char* name, float x) {
  return x > 0.f && std::isfinite(x) ? GBP_OK : bad_arg(fn, std::string(name) + " is not a positive number");
}
inline int need_number(const char* fn, const char* name, float x) { return std::isnan(x) ? bad_arg(fn, std::string(name) + " is NaN") : GBP_OK; }
constexpr uint64_t kMaxLanes = 0xffffff00ull;      // one lane per item, 32-bit lane index

}  // namespace stateless
}  // namespace gbp
