// The run-time logN as the kernels' compile-time LOGN, for the host code of both engines (helm_hip.hip, helm_shortint.hip).
#pragma once
#include <type_traits>

// f(std::integral_constant<int, LOGN>) for LO <= logN <= HI - the call site names the range, so it instantiates the kernels
// of that range and no other - and `outside` for any other logN.
template <int LO, int HI, class R, class F>
R with_logn(int logN, R outside, F &&f)
{
    if (logN == LO) return f(std::integral_constant<int, LO>{});
    if constexpr (LO < HI) return with_logn<LO + 1, HI>(logN, outside, f);
    else return outside;
}
