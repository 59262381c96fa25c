// A run-time integer as a template argument: with_const<1, 2, 3, 4>(nkc, [&](auto NK) { ... kernel<NK()> ... }) calls f exactly once,
// with std::integral_constant<int, V> of the listed V that equals v.  What happens to an unlisted v is part of the name:
//   with_const     - the LAST listed V takes every other value (the "default:" of the switches this replaced);
//   with_const_or  - f is not called and `otherwise` comes back (the launchers' strict form passes hipErrorInvalidValue, host_util.h).
// The value f returns comes back unchanged.  Plain C++17, no HIP types: tests/test_dispatch_host.py compiles this header alone with g++.
#pragma once
#include <type_traits>
#include <utility>

namespace stego {

template <int V, int... Vs, class F>
inline decltype(auto) with_const(int v, F&& f)
{
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V>{});
    } else {
        if (v == V) return f(std::integral_constant<int, V>{});
        return with_const<Vs...>(v, std::forward<F>(f));
    }
}

template <int V, int... Vs, class R, class F>
inline R with_const_or(int v, R otherwise, F&& f)
{
    if (v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Vs) == 0) return otherwise;
    else return with_const_or<Vs...>(v, otherwise, std::forward<F>(f));
}

}  // namespace stego
