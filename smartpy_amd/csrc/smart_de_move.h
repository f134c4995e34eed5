// smart_de_move.h -- the differential-evolution move the generational samplers share (smart_demcz.hip: smart_demcz_propose,
// smart_nsga2.hip: smart_nsga2_vary; smart_particle.hip: smart_particle_resample, which moves a child from its parent's own
// row with weight 0 and every jittered dimension marked as moved): the box of a call and the key of its draws as kernel arguments, the subspace
// crossover, the move of one row with its one reflection at the box, and the row of the launch matrix.  What differs stays
// in the two kernels: the base row, the two partner rows, the weight of their difference and where the fallback dimension
// is drawn.  The draw layout (include/smart_amd.h) is ABI: counter (row, generation, 2 + j, 0) belongs to dimension j, word 0
// against the crossover threshold, words 1 and 2 the jitter.
// ARITHMETIC.  The three units are compiled with -ffp-contract=off and this header adds no pragma of its own: every operation
// below is rounded once, in the order written, and each is correctly rounded.
#pragma once

#include "../../include/smart_amd.h"
#include "smart_philox.h"

namespace smart {

static_assert(SMART_DEMCZ_MAX_DIMS == 16 && SMART_NSGA2_MAX_DIMS == 16 && SMART_PARTICLE_MAX_DIMS == 16,
              "one DeBox for every unit that moves rows");
constexpr int kDeMaxDims = 16;

// the box of a call, by value inside the kernel arguments: slots from n_dims on hold 0
struct DeBox {
    double lo[kDeMaxDims], hi[kDeMaxDims], scale[kDeMaxDims];
    int columns[kDeMaxDims];
};

inline DeBox de_box(int n_dims, const double *lo, const double *hi, const double *scale, const int *columns)
{
    DeBox b;
    for (int j = 0; j < kDeMaxDims; ++j) {
        const bool live = j < n_dims;
        b.lo[j] = live ? lo[j] : 0.0, b.hi[j] = live ? hi[j] : 0.0, b.scale[j] = live ? scale[j] : 0.0;
        b.columns[j] = live ? columns[j] : 0;
    }
    return b;
}

// the generation and the seed's two halves: counter word 1 and the key of every draw of a call
struct DeKey {
    unsigned gen, k0, k1;
};

inline DeKey de_key(long generation, unsigned long long seed)
{
    return DeKey{(unsigned)generation, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)};
}

// which dimensions move: the crossover draw of each against C, the fallback dimension where none was drawn
__device__ __forceinline__ unsigned de_crossover(unsigned row, DeKey k, int d, unsigned long long C, int fallback)
{
    unsigned moved = 0;
    for (int j = 0; j < d; ++j) {
        const Philox4 w = philox4x32_10(row, k.gen, 2u + j, 0u, k.k0, k.k1);
        if ((unsigned long long)w.w[0] < C)
            moved |= 1u << j;
    }
    if (moved == 0)
        moved = 1u << fallback;
    return moved;
}

// y_out = base, and in the dimensions of `moved` base + (weight (a - b) + jitter), reflected once at lo, then once at hi
// -> whether a moved dimension is still outside the box
__device__ __forceinline__ bool de_move(unsigned row, DeKey k, int d, unsigned moved, const DeBox &box,
                                        const double *base, const double *a, const double *b, double weight, double *y_out)
{
    bool out = false;
    for (int j = 0; j < d; ++j) {
        double y = base[j];
        if ((moved >> j) & 1u) {
            const Philox4 w = philox4x32_10(row, k.gen, 2u + j, 0u, k.k0, k.k1);
            const double eps = box.scale[j] * (2.0 * u53(w.w[1], w.w[2]) - 1.0);
            double t = a[j] - b[j];
            t = weight * t;
            t = t + eps;
            y = y + t;
            const double lo = box.lo[j], hi = box.hi[j];
            if (y < lo)
                y = 2.0 * lo - y;
            if (y > hi)
                y = 2.0 * hi - y;
            if (!(y >= lo && y <= hi))
                out = true;
        }
        y_out[j] = y;
    }
    return out;
}

// the launch matrix: the moved row, or its base row where the move left the box (a row the model can run)
__device__ __forceinline__ void de_launch_row(int d, const DeBox &box, bool out, const double *base, const double *y_out,
                                              double *row)
{
    for (int j = 0; j < d; ++j)
        row[box.columns[j]] = out ? base[j] : y_out[j];
}

} // namespace smart
