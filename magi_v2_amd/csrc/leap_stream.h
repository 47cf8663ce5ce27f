// Pieces of the VALU streaming kernel's body (leap_stream_body.h) shared by leap.hip (k_stream) and leap_group.hip (k_stream_group):
// the transposed butterfly of the row-type products and the wave split of a block.  Included inside an anonymous namespace.
#pragma once

// Transposed butterfly: v[0..8) per lane -> every lane returns the 64-lane sum of v[lane >> 3].
// Halving steps hand half of the values to the partner (v_permlane32/16_swap move both halves in one
// instruction pair), so 8 row sums cost 7 exchanges + 3 plain steps instead of 8 x 6.
__device__ __forceinline__ double swap_add32(double a, double b) {
    unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ double swap_add16(double a, double b) {
    unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ double tsum8(const double (&v)[8], int lane) {
    // lanes 32..63 keep rows 4..7, lanes 0..31 rows 0..3
    const double s0 = swap_add32(v[0], v[4]), s1 = swap_add32(v[1], v[5]), s2 = swap_add32(v[2], v[6]), s3 = swap_add32(v[3], v[7]);
    // odd rows of 16 lanes keep the upper two of those
    const double u0 = swap_add16(s0, s2), u1 = swap_add16(s1, s3);
    // lanes with bit 3 set keep u1 (partner: row_mirror, which flips bit 3)
    const bool hi8 = (lane & 8) != 0;
    const double keep = hi8 ? u1 : u0, send = hi8 ? u0 : u1;
    double w = keep + dpp_f64<0x140>(send);
    w += dpp_f64<0x141>(w);   // row_half_mirror (stays inside the 8-lane group)
    w += dpp_f64<0x4E>(w);
    w += dpp_f64<0xB1>(w);
    return w;
}

#ifndef MAGI_ST_WAVES
#define MAGI_ST_WAVES 4
#endif
constexpr int ST_WAVES = MAGI_ST_WAVES;        // waves per block task
constexpr int ST_RW = MAGI_TB / ST_WAVES;      // rows of the block per wave
