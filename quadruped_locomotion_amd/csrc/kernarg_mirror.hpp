// The check that goes with coop::kernel_arguments_again (balance_coop.hpp): a struct laid over a kernel's argument segment is
// written by hand, and nothing but these static_asserts ties it to the kernel's signature.
#pragma once

#include <cstddef>
#include <tuple>
#include <type_traits>

namespace qlamd {

// Where a kernel's parameters lie in its argument segment: each at its natural alignment, in the order of the signature
template <class F> struct KernargLayout;
template <class... P> struct KernargLayout<void (*)(P...)> {
  static constexpr size_t count = sizeof...(P);
  static constexpr size_t offset(size_t k) { // (k == count: the length of the segment's explicit part)
    const size_t size[] = {sizeof(P)...}, align[] = {alignof(P)...};
    size_t o = 0;
    for (size_t j = 0; j < k; j++) o = (o + align[j] - 1) / align[j] * align[j] + size[j];
    return k < count ? (o + align[k] - 1) / align[k] * align[k] : o;
  }
  template <size_t k> using type = std::tuple_element_t<k, std::tuple<P...>>;
};

} // namespace qlamd

// QL_KERNARG_MIRROR(Layout, Struct, whole, members...): the listed members of Struct, in this order, have the types and the
// places of the first parameters of the kernel behind Layout (a KernargLayout); whole: they are all of its parameters and
// Struct ends where they end.  Up to 12 members.
#define QL_KA_ONE(L, S, k, m)                                                                                                  \
  static_assert(std::is_same<L::type<(k)>, decltype(S::m)>::value, #S "::" #m " has not the type of the kernel's parameter at its place in the list"); \
  static_assert(L::offset(k) == offsetof(S, m), #S "::" #m " does not lie where the kernel's parameter at its place in the list lies");
#define QL_KA_1(L, S, n, m) QL_KA_ONE(L, S, n - 1, m)
#define QL_KA_2(L, S, n, m, ...) QL_KA_ONE(L, S, n - 2, m) QL_KA_1(L, S, n, __VA_ARGS__)
#define QL_KA_3(L, S, n, m, ...) QL_KA_ONE(L, S, n - 3, m) QL_KA_2(L, S, n, __VA_ARGS__)
#define QL_KA_4(L, S, n, m, ...) QL_KA_ONE(L, S, n - 4, m) QL_KA_3(L, S, n, __VA_ARGS__)
#define QL_KA_5(L, S, n, m, ...) QL_KA_ONE(L, S, n - 5, m) QL_KA_4(L, S, n, __VA_ARGS__)
#define QL_KA_6(L, S, n, m, ...) QL_KA_ONE(L, S, n - 6, m) QL_KA_5(L, S, n, __VA_ARGS__)
#define QL_KA_7(L, S, n, m, ...) QL_KA_ONE(L, S, n - 7, m) QL_KA_6(L, S, n, __VA_ARGS__)
#define QL_KA_8(L, S, n, m, ...) QL_KA_ONE(L, S, n - 8, m) QL_KA_7(L, S, n, __VA_ARGS__)
#define QL_KA_9(L, S, n, m, ...) QL_KA_ONE(L, S, n - 9, m) QL_KA_8(L, S, n, __VA_ARGS__)
#define QL_KA_10(L, S, n, m, ...) QL_KA_ONE(L, S, n - 10, m) QL_KA_9(L, S, n, __VA_ARGS__)
#define QL_KA_11(L, S, n, m, ...) QL_KA_ONE(L, S, n - 11, m) QL_KA_10(L, S, n, __VA_ARGS__)
#define QL_KA_12(L, S, n, m, ...) QL_KA_ONE(L, S, n - 12, m) QL_KA_11(L, S, n, __VA_ARGS__)
#define QL_KA_COUNT(_1, _2, _3, _4, _5, _6, _7, _8, _9, _10, _11, _12, n, ...) n
#define QL_KA_CAT(a, b) a##b
#define QL_KA_EACH(n) QL_KA_CAT(QL_KA_, n)
#define QL_KERNARG_MIRROR_N(L, S, whole, n, ...)                                                                            \
  static_assert((whole) ? L::count == n : L::count >= n, #S " does not list the kernel's number of parameters"); \
  QL_KA_EACH(n)(L, S, n, __VA_ARGS__)                                                                                       \
  static_assert(!(whole) || L::offset(L::count) == sizeof(S), #S " is not as long as the kernel's parameters")
#define QL_KERNARG_MIRROR(L, S, whole, ...) \
  QL_KERNARG_MIRROR_N(L, S, whole, QL_KA_COUNT(__VA_ARGS__, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0), __VA_ARGS__)
