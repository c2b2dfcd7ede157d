// dispatch_check.cpp — gigl_amd/csrc/dispatch.h on the CPU (g++ -std=c++17, nothing from HIP): every listed value reaches
// its own tag, an unlisted one the LAST tag, f runs exactly once, and its return value comes through.
//   g++ -std=c++17 -Igigl_amd/csrc tests/c/dispatch_check.cpp -o dispatch_check && ./dispatch_check
#include "dispatch.h"

#include <cstdio>
#include <initializer_list>
#include <type_traits>

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// v -> the tag dispatch_int<Ns...> hands to f; `want` = what the ladder `if (v == N0) .. else <last>` picks
template <int... Ns>
static void check_ints(std::initializer_list<int> listed, std::initializer_list<int> unlisted, int last) {
  for (int v : listed) {
    int calls = 0;
    const int got = dispatch_int<Ns...>(v, [&](auto tag) {
      static_assert(std::is_same<typename decltype(tag)::value_type, int>::value, "an int tag");
      ++calls;
      return decltype(tag)::value * 10 + 1;  // (a value that only this tag gives)
    });
    CHECK(calls == 1);
    CHECK(got == v * 10 + 1);
  }
  for (int v : unlisted) {
    int calls = 0, seen = -1;
    dispatch_int<Ns...>(v, [&](auto tag) {  // (void return)
      ++calls;
      seen = decltype(tag)::value;
    });
    CHECK(calls == 1);
    CHECK(seen == last);
  }
}

template <typename T>
static int type_id() {
  return std::is_same<T, float>::value ? 100 : std::is_same<T, short>::value ? 200 : std::is_same<T, double>::value ? 300 : -1;
}

int main() {
  check_ints<1, 2, 4>({1, 2, 4}, {0, 3, 5, -1, 1 << 30}, 4);
  check_ints<1, 2, 3, 4>({1, 2, 3, 4}, {0, 5, -7}, 4);
  check_ints<8, 16, 32, 64>({8, 16, 32, 64}, {0, 1, 24, 65, 128}, 64);
  check_ints<2, 1>({2, 1}, {0, 3}, 1);  // (the order is the caller's: the last LISTED value is the fallback)
  check_ints<7>({7}, {0, 8}, 7);

  // the tag is a compile-time constant inside f
  dispatch_int<1, 2, 4>(2, [](auto tag) {
    constexpr int V = decltype(tag)::value;
    static_assert(V == 1 || V == 2 || V == 4, "only the listed values are instantiated");
    char a[V];
    (void)a;
  });

  // dispatch_type: index i -> the i-th type, anything else -> the last
  const int want_two[] = {100, 200};
  for (int i = 0; i < 2; ++i) {
    int calls = 0;
    const int got = dispatch_type<float, short>(i, [&](auto t) {
      ++calls;
      return type_id<typename decltype(t)::type>();
    });
    CHECK(calls == 1);
    CHECK(got == want_two[i]);
  }
  for (int i : {2, 3, -1, 1 << 20}) {
    int calls = 0;
    const int got = dispatch_type<float, short>(i, [&](auto t) {
      ++calls;
      return type_id<typename decltype(t)::type>();
    });
    CHECK(calls == 1);
    CHECK(got == 200);
  }
  const int want_three[] = {100, 200, 300, 300, 300};
  for (int i = 0; i < 5; ++i) {
    int calls = 0, seen = 0;
    dispatch_type<float, short, double>(i, [&](auto t) {  // (void return)
      ++calls;
      seen = type_id<typename decltype(t)::type>();
    });
    CHECK(calls == 1);
    CHECK(seen == want_three[i]);
  }

  // dispatch_bool
  for (bool b : {false, true}) {
    int calls = 0;
    const int got = dispatch_bool(b, [&](auto tag) {
      constexpr bool B = decltype(tag)::value;
      ++calls;
      return B ? 7 : 3;
    });
    CHECK(calls == 1);
    CHECK(got == (b ? 7 : 3));
    int seen = -1;
    dispatch_bool(b, [&](auto tag) { seen = decltype(tag)::value ? 1 : 0; });  // (void return)
    CHECK(seen == (b ? 1 : 0));
  }

  // nested, as the launch sites use it: each axis keeps its own tag, the innermost body runs once
  for (int dt : {0, 1})
    for (int p : {1, 2, 3, 4, 9})
      for (int h : {1, 2, 4, 3})
        for (bool e : {false, true}) {
          int calls = 0;
          const long got = dispatch_type<float, short>(dt, [&](auto t) {
            return dispatch_int<1, 2, 3, 4>(p, [&](auto pp) {
              return dispatch_int<1, 2, 4>(h, [&](auto hh) {
                return dispatch_bool(e, [&](auto ee) {
                  ++calls;
                  return (long)type_id<typename decltype(t)::type>() * 1000 + decltype(pp)::value * 100 +
                         decltype(hh)::value * 10 + (decltype(ee)::value ? 1 : 0);
                });
              });
            });
          });
          const long want = (dt == 0 ? 100 : 200) * 1000L + (p > 4 ? 4 : p) * 100 + (h == 3 ? 4 : h) * 10 + (e ? 1 : 0);
          CHECK(calls == 1);
          CHECK(got == want);
        }

  // a reference comes through as a reference
  int slot_a = 0, slot_b = 0;
  int& r = dispatch_bool(true, [&](auto tag) -> int& { return decltype(tag)::value ? slot_a : slot_b; });
  r = 5;
  CHECK(slot_a == 5 && slot_b == 0);

  if (failures) return 1;
  std::printf("dispatch OK\n");
  return 0;
}
