// smart_order_keys.h -- doubles as ORDER-PRESERVING 64-BIT KEYS: unsigned order of the keys = numeric order of the
// doubles, every NaN one key above +inf, both zeros one key, and one key above them all for padding.  What the kernels
// that sort or select compare: smart_quantiles.hip, smart_ensemble_scores.hip, smart_dynia.hip and smart_pawn.hip along
// the sample axis (with smart_order_stats.h, the network and the scan of those that sort, and smart_key_select.h, the
// k-th key by bisection), smart_flow_duration.hip along time.
#pragma once
#include <hip/hip_runtime.h>

namespace smart {

constexpr unsigned long long kKeyNaN = 0xfff8000000000000ull;  // above +inf (0xfff0...), below the padding
constexpr unsigned long long kKeyPlusInf = 0xfff0000000000000ull;   // value_key(+inf): a finite value lies below
constexpr unsigned long long kKeyMinusInf = 0x000fffffffffffffull;  // value_key(-inf): a finite value lies above
constexpr unsigned long long kKeyPad = 0xffffffffffffffffull;
constexpr unsigned long long kKeyZero = 0x8000000000000000ull;

__device__ inline unsigned long long value_key(double x)
{
    if (x != x)
        return kKeyNaN;
    if (x == 0.0)
        return kKeyZero;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | kKeyZero);
}

__device__ inline double key_value(unsigned long long k)
{
    if (k >= kKeyNaN)
        return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? (k & ~kKeyZero) : ~k));
}

} // namespace smart
