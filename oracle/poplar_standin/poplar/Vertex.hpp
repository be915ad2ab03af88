// poplar/Vertex.hpp — STAND-IN, TEST INFRASTRUCTURE ONLY (oracle/ref_vertex_adapter.cpp, `make -C oracle ref`).
//
// The reference's vertex classes (ba/gbp_codelets.cpp) are plain C++ over float / unsigned / int; the Poplar SDK only
// supplies the wrappers their fields are declared with.  This header restates those wrappers' documented access semantics
// over a caller-supplied pointer and nothing else — no graph, no tile, no scheduling:
//   Input<T> / Output<T> / InOut<T>   one element: converts to T& (const T& for Input), operator* and operator-> reach it,
//                                     compound assignment goes to the element (`weaken_flag -= 1`)
//   Input<Vector<T>> / ...            a contiguous run: operator[] and size(); the element reference of an Input is
//                                     not const, because the codelets build `Mat<float>(&field[0], ...)` from inputs
//   Vertex                            the empty base class
// Every wrapped type is an arithmetic type, so the TYPE of every expression of the codelets (`0.5 * Nstds` is a double,
// `std::sqrt(meas_variance)` the float overload, `1 - damping` a float) is decided by C++ exactly as with the SDK's
// wrappers; ref_vertex_adapter.cpp static_asserts the ones the arithmetic depends on.
// bind() is the stand-in's only addition: it points a field at the caller's memory.
#ifndef GBP_ORACLE_POPLAR_STANDIN_VERTEX_HPP
#define GBP_ORACLE_POPLAR_STANDIN_VERTEX_HPP
#include <cstddef>

namespace poplar {

class Vertex {};

template <typename T> class Vector {};

namespace standin {
template <typename T> class ScalarRef {
 protected:
  T* p_ = nullptr;
 public:
  void bind(T* p) { p_ = p; }
};
template <typename T> class VectorRef {
 protected:
  T* p_ = nullptr;
  std::size_t n_ = 0;
 public:
  void bind(T* p, std::size_t n) { p_ = p; n_ = n; }
  std::size_t size() const { return n_; }
  T& operator[](std::size_t i) const { return p_[i]; }
};
}  // namespace standin

template <typename T> class Input : public standin::ScalarRef<T> {
 public:
  operator const T&() const { return *this->p_; }
  const T& operator*() const { return *this->p_; }
  const T* operator->() const { return this->p_; }
};
template <typename T> class InOut : public standin::ScalarRef<T> {
 public:
  operator T&() const { return *this->p_; }
  T& operator*() const { return *this->p_; }
  T* operator->() const { return this->p_; }
  InOut& operator=(const T& v) { *this->p_ = v; return *this; }
};
template <typename T> class Output : public InOut<T> {
 public:
  Output& operator=(const T& v) { *this->p_ = v; return *this; }
};

template <typename T> class Input<Vector<T>> : public standin::VectorRef<T> {};
template <typename T> class InOut<Vector<T>> : public standin::VectorRef<T> {};
template <typename T> class Output<Vector<T>> : public standin::VectorRef<T> {};

}  // namespace poplar
#endif
