// lazy.hpp -- what the streaming probes of lazy.hip (LazyBisectCost) and lazy_flip.hip (LazyFlipBisectCost) share: the comparison of
// a cost with the Float64 bisection value, the chunk geometry, the per-chunk prefix tables in shared memory, the primary model's
// formula, the owner stream and the bound of a primary model with per-part alpha.
#pragma once
#include "csr.hpp"
#include "model.hpp"
#include "dp.hpp"
#include <type_traits>
#include <vector>

namespace cpk {

__device__ __forceinline__ bool lz_le(int64_t v, double c)
{
    if (c != c) return false;
    if (c >= 9223372036854775808.0) return true;
    if (c < -9223372036854775808.0) return false;
    return v <= (int64_t)floor(c);
}
__device__ __forceinline__ bool lz_le(double v, double c) { return v <= c; }

constexpr int LZ_T = 1024;             // lanes
constexpr int LZ_E = 16;               // link entries per lane and chunk
constexpr int LZ_CH = LZ_T * LZ_E;

struct LazyShared {
    int32_t tbase[LZ_T];               // exclusive prefix of the per-lane flag counts
    uint16_t tmask[LZ_T];              // flags of the lane's 16 entries
    int32_t wsum[LZ_T / 64];
    int32_t red[LZ_T / 64];
    int32_t total;
};

// #flagged entries in [qa, qa + i)
__device__ __forceinline__ int32_t lz_prefix(const LazyShared &S, int32_t i)
{
    if (i >= LZ_CH) return S.total;
    int t = i >> 4, r = i & 15;
    return S.tbase[t] + __popc((uint32_t)S.tmask[t] & ((1u << r) - 1u));
}

struct LazyPlaidShared {
    uint32_t tbase[LZ_T];              // exclusive prefix of the per-lane counts, local | remote << 16
    uint16_t tml[LZ_T], tmr[LZ_T];     // flags of the lane's 16 entries: new and local, new and remote
    uint32_t wsum[LZ_T / 64];
    int32_t red[LZ_T / 64], ncmp[LZ_T / 64];
    uint32_t total;
};

// (#local | #remote << 16) flagged entries in [qa, qa + i)
__device__ __forceinline__ uint32_t lz_prefix(const LazyPlaidShared &S, int32_t i)
{
    if (i >= LZ_CH) return S.total;
    int t = i >> 4;
    uint32_t low = (1u << (i & 15)) - 1u;
    return S.tbase[t] + (uint32_t)__popc((uint32_t)S.tml[t] & low) + ((uint32_t)__popc((uint32_t)S.tmr[t] & low) << 16);
}

// kind 8 of dm_apply, slot for slot (the kernel needs no other kind; the whole switch costs the Float64 kernel its registers)
template <typename TC>
__device__ __forceinline__ TC lz_primary(const DevModel<TC> &m, TC alpha, int64_t nv, int64_t np, int64_t nl, int64_t nr)
{
    return cadd(cadd(cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN])), cmulc(nl, m.p[CP_P_LOCAL_NET])),
                cmulc(nr, m.p[CP_P_REMOTE_NET]));
}

// lazy.hip: eown[q] = owner[row[q]]; the 16 entries behind N are written too (the probe's 16-byte loads reach into them)
__global__ void __launch_bounds__(256) k_lazy_eown(int64_t N, int64_t Npad, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                                                   int32_t *__restrict__ eown);

// bound_stripe(A, K, Pi, f) of a primary model with per-part alpha, the reference tests' FunkyPrimaryConnectivityModel
// (test_Partitioners.jl:43-48): (minimum, maximum) of (minimum(alpha), maximum(alpha), maximum_k ocl(1, n + 1, k)), k = 1 .. K.
// The oracle takes part numbers up to Pi.K, so Pi is widened to K parts (the added ones own no row).
template <typename TC>
int32_t lazy_plaid_funky_bound(cp_csr_s *A, int64_t K, const cp_model_t *mdl, const cp_rowpart_t *Pi, double *lo, double *hi)
{
    CP_REQUIRE(mdl->n_alpha_k >= K, CP_EINVAL, "bound_stripe: fewer per-part alphas than parts");
    cp_rowpart_t wide;
    std::vector<int64_t> wspl;
    wide.K = K; wide.asg = Pi->asg; wide.spl = nullptr;
    if (!Pi->asg) {
        wspl.assign(Pi->spl, Pi->spl + Pi->K + 1);
        wspl.resize((size_t)K + 1, A->m + 1);
        wide.spl = wspl.data();
    }
    std::vector<int64_t> one((size_t)K, 1), np1((size_t)K, A->n + 1), ks((size_t)K);
    for (int64_t k = 0; k < K; k++) ks[(size_t)k] = k + 1;
    std::vector<TC> v((size_t)K);
    const bool i64 = std::is_same<TC, int64_t>::value;
    int32_t rc = cp_oracle_eval(A, mdl, &wide, CP_HINT_STEP, K, one.data(), np1.data(), ks.data(), i64 ? (int64_t *)v.data() : nullptr,
                                i64 ? nullptr : (double *)v.data());
    if (rc != CP_OK) return rc;
    const TC *al = (const TC *)mdl->alpha_k;
    TC amin = al[0], amax = al[0], fmax = v[0];
    for (int64_t i = 1; i < mdl->n_alpha_k; i++) { amin = std::min(amin, al[i]); amax = std::max(amax, al[i]); }
    for (int64_t k = 1; k < K; k++) fmax = std::max(fmax, v[(size_t)k]);
    *lo = (double)std::min(amin, std::min(amax, fmax)); *hi = (double)std::max(amin, std::max(amax, fmax));
    return CP_OK;
}

}  // namespace cpk
