// The gate of the mixture-of-experts layer for ONE token on ONE wave, shared by moe.hip (gate_rows_kernel: any number of
// tokens, training) and moe_rows.hip (moe_route_rows_kernel: the few rows of a decoding step): fp32 softmax over E <= 256
// experts, top-2 by the project's ranking rule, the two weights normalised to sum 1.  One code path: both kernels give the
// same bits for the same fp32 logits.
#pragma once
#include "common.h"

constexpr int MOE_E_MAX = 256;

// higher fp32 gate VALUE first; among exactly equal values the LOWER expert index
__device__ __forceinline__ bool moe_ranks_before(float va, int ia, float vb, int ib) {
    return va > vb || (va == vb && ia < ib);
}

// `logit(e)`: the fp32 logit of expert e of this wave's token.  g_row: where the E gate values go, or nullptr.
// All 64 lanes call; every lane returns the same bi (experts) and bw (normalised weights).
template <typename LOGIT>
__device__ __forceinline__ void moe_gate_token(LOGIT logit, int lane, int E, float* __restrict__ g_row, int (&bi)[2], float (&bw)[2]) {
    float v[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        v[j] = e < E ? logit(e) : -INFINITY;
        mx = fmaxf(mx, v[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = (lane + 64 * j) < E ? expf(v[j] - mx) : 0.f;
        sum += v[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    float bv[2];
    int taken = -1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float cv = -1.f;
        int ci = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            if (k == 0) {
                v[j] = v[j] / sum;
                if (g_row != nullptr && e < E) g_row[e] = v[j];
            }
            if (e < E && e != taken && moe_ranks_before(v[j], e, cv, ci)) {
                cv = v[j];
                ci = e;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(cv, o, 64);
            const int oi = __shfl_xor(ci, o, 64);
            if (moe_ranks_before(ov, oi, cv, ci)) {
                cv = ov;
                ci = oi;
            }
        }
        if (ci >= E) {  // nothing ranked (a row of NaN logits): a valid expert all the same, the tables are indexed by it
            ci = (k == 1 && taken == 0) ? 1 : 0;
            cv = 0.f;
        }
        bv[k] = cv;
        bi[k] = ci;
        taken = ci;
    }
    const float den = bv[0] + bv[1];
    bw[0] = bv[0] / den;
    bw[1] = bv[1] / den;
}
