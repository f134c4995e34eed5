// Where a time-sliced launch cuts the time axis.  Plain C++ (no HIP header needed): the host, the kernels and a
// stand-alone test program include this one file, and everything in it is integer arithmetic, so the three cannot
// disagree about a cut.
//
// A launch of n_seg slices cuts the n_all intervals of the axis (warm-up intervals, then report intervals) at
// slice_cut(n_all, k, n_seg, taper), k = 0 ... n_seg: slice k is [cut(k), cut(k + 1)).
//   taper == 0   equal slices, n_all * k / n_seg.
//   taper != 0   long slices first, short ones at the end (the shape of guided self-scheduling): the chains of a launch
//                advance within about one slice of each other, so the SIMDs run dry over roughly the wall time of the
//                LAST slice, and that is the one that should be short; the number of hand-overs stays what it was.
//                The first n_seg - m slices have weight 1, the last m = n_seg / 4 (six at the most) fall geometrically
//                by 0.6 a slice (24 slices: the last six are 0.6 ... 0.047 of an early one, the last 0.24 % of the
//                axis).  The cuts are the prefix sums of the weights scaled to n_all, rounded down.  Where that would
//                make a slice shorter than four intervals (or, by the rounding, leave the last one above half the
//                first), or with fewer than eight slices, the cuts are the equal ones.
//                (0.6 against 0.75, and n_seg / 4 against n_seg / 3: profiles/slice_taper.txt)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMART_CUTS_FN __host__ __device__ constexpr
#else
#define SMART_CUTS_FN constexpr
#endif

namespace smart {

constexpr long kCutUnit = 1024;  // weight of an early slice
constexpr int kCutTail = 6;      // the longest tail: 1024 * 0.6^i, i = 1 ... 6, and their prefix sums
constexpr int kCutMinSlices = 8; // fewer slices than this are never tapered
constexpr long kCutMinLen = 4;   // a tapered launch has no slice shorter than this many intervals

// prefix sum of the tail's weights: of its first j slices, j = 0 ... kCutTail (a switch, not a table: a table indexed
// on the device would be a load from constant memory)
SMART_CUTS_FN long cut_tail_sum(int j)
{
    // weights 614 369 221 133 80 48
    return j <= 0 ? 0 : j == 1 ? 614 : j == 2 ? 983 : j == 3 ? 1204 : j == 4 ? 1337 : j == 5 ? 1417 : 1465;
}

// slices in the tail of a launch of n_seg
SMART_CUTS_FN int cut_tail_len(long n_seg)
{
    const long m = n_seg / 4;
    return (int)(m < kCutTail ? m : kCutTail);
}

// the tapered cut itself, for a launch the taper applies to (slice_taper_applies): two multiplications and one division
SMART_CUTS_FN long slice_cut_tapered(long n_all, long k, long n_seg)
{
    const int m = cut_tail_len(n_seg);
    const long n_early = n_seg - m;
    const long total = n_early * kCutUnit + cut_tail_sum(m);
    const long upto = k <= n_early ? k * kCutUnit : n_early * kCutUnit + cut_tail_sum((int)(k - n_early));
    return k >= n_seg ? n_all : n_all * upto / total;
}

// does the taper apply to a launch of n_seg slices over n_all intervals?  (the early slices are floor(x) or ceil(x)
// intervals, x = n_all * 1024 / total; the tail is looked at slice by slice)
SMART_CUTS_FN bool slice_taper_applies(long n_all, long n_seg)
{
    if (n_seg < kCutMinSlices || n_all < n_seg * kCutMinLen)
        return false;
    const int m = cut_tail_len(n_seg);
    const long total = (n_seg - m) * kCutUnit + cut_tail_sum(m);
    if (n_all * kCutUnit / total < kCutMinLen)
        return false;
    for (long k = n_seg - m; k < n_seg; ++k)
        if (slice_cut_tapered(n_all, k + 1, n_seg) - slice_cut_tapered(n_all, k, n_seg) < kCutMinLen)
            return false;
    // (at a few intervals a slice the rounding can leave the last one above half the first: not a taper worth its name)
    return 2 * (n_all - slice_cut_tapered(n_all, n_seg - 1, n_seg)) <= slice_cut_tapered(n_all, 1, n_seg);
}

// first interval of slice k (k == n_seg: the end of the axis)
SMART_CUTS_FN long slice_cut(long n_all, long k, long n_seg, int taper)
{
    return taper && slice_taper_applies(n_all, n_seg) ? slice_cut_tapered(n_all, k, n_seg) : n_all * k / n_seg;
}

} // namespace smart
