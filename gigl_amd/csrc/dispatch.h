// dispatch.h — a run-time value picks a compile-time tag (host only; nothing from HIP).
//
// Every entry point validates its arguments first; the dispatchers then call f exactly once with the tag of the FIRST listed
// value equal to v, or of the LAST listed value when none is (the trailing `else` of a hand-written ladder).  They return
// what f returns (every tag must give the same type; void is fine).
//
//   dispatch_int<1, 2, 4>(heads, [&](auto hh) { constexpr int H = decltype(hh)::value; launch<H>(...); });
//   dispatch_type<float, __half>(dtype, [&](auto t) { using T = typename decltype(t)::type; launch<T>(...); });
#pragma once

#include <type_traits>
#include <utility>

template <typename T>
struct type_tag {
  using type = T;
};

template <int N0, int... Ns, typename F>
inline decltype(auto) dispatch_int(int v, F&& f) {
  if constexpr (sizeof...(Ns) == 0) {
    return f(std::integral_constant<int, N0>{});
  } else {
    if (v == N0) return f(std::integral_constant<int, N0>{});
    return dispatch_int<Ns...>(v, std::forward<F>(f));
  }
}

// index 0 -> T0, 1 -> T1, ...; any other index -> the last type
template <typename T0, typename... Ts, typename F>
inline decltype(auto) dispatch_type(int index, F&& f) {
  if constexpr (sizeof...(Ts) == 0) {
    return f(type_tag<T0>{});
  } else {
    if (index == 0) return f(type_tag<T0>{});
    return dispatch_type<Ts...>(index - 1, std::forward<F>(f));
  }
}

template <typename F>
inline decltype(auto) dispatch_bool(bool b, F&& f) {
  if (b) return f(std::true_type{});
  return f(std::false_type{});
}
