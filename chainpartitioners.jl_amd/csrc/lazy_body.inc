// lazy_body.inc -- the body of the LazyBisectCost kernels of lazy.hip, included once per kernel.  The including kernel provides
// M, n, N, K, pos, prev, c_lo, c_hi, eps, spl, spl_hi, nprobes, the shared LazyShared S, and
//   constexpr bool SEP; const int32_t *pin;      SEP: the pin count of a column range comes from the prefix array `pin`
//                                                (the symmetric specialisation), otherwise from pos itself
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // spl / spl_hi live in global memory; every store is made by lane 0 only and read back after a barrier
    if (tid == 0) {
        for (int64_t k = 0; k <= K; k++) { spl[k] = 0; spl_hi[k] = n + 1; }
        spl[0] = 1; spl_hi[0] = 1;                                     // :146-150
    }
    for (int64_t k = 1; k <= K; k++) {                                 // :233-235  c_lo = max(c_lo, f(0, 0, 0, k))
        double v = (double)dm_apply(M, dm_alpha(M, k), (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0);
        c_lo = c_lo < v ? v : c_lo;
    }
    int64_t probes = 0;
    bool first = true, stuck = false;
    while (c_lo * (1 + eps) < c_hi) {                                  // :237-247, :249-257
        double c = (c_lo + c_hi) / 2;
        probes++;
        bool res = true;
        int64_t k = 1;
        int32_t j0 = 0;                                                // 0-based first column of the open part
        int32_t col = 0;                                               // next column to close
        int32_t qs = 0;                                                // next link entry to read
        int32_t cnt0 = 0;                                              // nets of [j0, col) plus flagged entries in [pos[col], qs)
        if (tid == 0) spl[0] = 1;
        while (col < n) {
            // ---- one chunk of link entries [qs, qe), loaded as aligned 16-byte pieces
            int32_t qa = qs & ~3;
            int32_t qe = (int32_t)((int64_t)qa + LZ_CH < N ? (int64_t)qa + LZ_CH : N);
            uint32_t mask = 0;
            {
                int32_t b = qa + tid * LZ_E;
#pragma unroll
                for (int v4 = 0; v4 < LZ_E / 4; v4++) {
                    int32_t x = b + 4 * v4;
                    if (x < qe) {                                      // arrays are padded by 8 entries
                        int4 v = *reinterpret_cast<const int4 *>(prev + x);
                        if (x >= qs && x < qe && v.x < j0) mask |= 1u << (4 * v4);
                        if (x + 1 >= qs && x + 1 < qe && v.y < j0) mask |= 1u << (4 * v4 + 1);
                        if (x + 2 >= qs && x + 2 < qe && v.z < j0) mask |= 1u << (4 * v4 + 2);
                        if (x + 3 >= qs && x + 3 < qe && v.w < j0) mask |= 1u << (4 * v4 + 3);
                    }
                }
            }
            int32_t mine = __popc(mask), incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { int32_t pv = __shfl_up(incl, o); if (lane >= o) incl += pv; }
            if (lane == 63) S.wsum[wave] = incl;
            __syncthreads();
            int32_t wbase = 0;
            for (int w = 0; w < wave; w++) wbase += S.wsum[w];
            S.tbase[tid] = wbase + incl - mine;
            S.tmask[tid] = (uint16_t)mask;
            if (tid == LZ_T - 1) S.total = wbase + incl;
            __syncthreads();
            // ---- close the columns that end inside the chunk, 1024 at a time
            bool restarted = false;
            bool checks = !first || k < K;                             // probe_init stops checking once k == K (:171)
            while (col < n) {
                int32_t c_me = col + tid;
                int32_t e = (c_me < n) ? pos[c_me + 1] : INT32_MAX;
                bool complete = c_me < n && e <= qe;
                bool exceed = false;
                if (complete && checks) {
                    int64_t nn = (int64_t)cnt0 + lz_prefix(S, e - qa);
                    TC v = dm_apply(M, dm_alpha(M, k), (int64_t)(c_me - j0 + 1), (int64_t)(SEP ? pin[c_me + 1] - pin[j0] : e - pos[j0]), nn, (int64_t)0);
                    exceed = !lz_le(v, c);
                }
                // first exceeding column and number of complete columns of this batch
                unsigned long long em = __ballot(exceed), cm = __ballot(complete);
                if (lane == 0) { S.red[wave] = em ? (wave * 64 + __ffsll((long long)em) - 1) : INT32_MAX; S.wsum[wave] = __popcll(cm); }
                __syncthreads();
                int32_t fx = INT32_MAX, ncomp = 0;
                for (int w = 0; w < LZ_T / 64; w++) { fx = S.red[w] < fx ? S.red[w] : fx; ncomp += S.wsum[w]; }
                __syncthreads();
                if (fx != INT32_MAX) {
                    // ---- split in front of column cx (:208-219): the column opens the next part on its own
                    int32_t cx = col + fx;
                    int32_t deg = pos[cx + 1] - pos[cx];
                    int32_t dpin = SEP ? pin[cx + 1] - pin[cx] : deg;
                    bool fail = false;
                    while (true) {
                        if (!first && k == K) { fail = true; break; }  // :209-211
                        if (tid == 0) spl[k] = (int64_t)cx + 1;
                        j0 = cx;
                        k += 1;
                        bool again = (!first || k < K) &&
                                     !lz_le(dm_apply(M, dm_alpha(M, k), (int64_t)1, (int64_t)dpin, (int64_t)deg, (int64_t)0), c);
                        if (!again) break;
                    }
                    if (fail) { res = false; col = (int32_t)n; restarted = true; break; }
                    col = cx + 1;
                    qs = pos[cx + 1];
                    cnt0 = deg;
                    restarted = true;
                    break;
                }
                col += ncomp;
                if (ncomp < LZ_T) break;                               // the next column ends beyond the chunk
            }
            if (!restarted) {
                cnt0 += S.total;                                       // everything flagged in [qs, qe) belongs to [j0, col]
                qs = qe;
            }
            __syncthreads();
        }
        if (res) {
            if (first) {                                               // :180  res = k < K || f(...) <= c
                int64_t nv = n - j0, np = (n > 0 ? (SEP ? (int64_t)pin[n] - pin[j0] : (int64_t)pos[n] - pos[j0]) : 0);
                res = k < K || lz_le(dm_apply(M, dm_alpha(M, K), nv, np, (int64_t)cnt0, (int64_t)0), c);
            }
            if (tid == 0) for (int64_t t = k; t <= K; t++) spl[t] = n + 1;    // :181-184 / :221-224
        }
        __syncthreads();
        // no bound moved: the reference would repeat this probe forever (non-positive bounds); block-uniform exit
        if ((res ? c_hi : c_lo) == c || probes > 4096) { stuck = true; break; }
        if (res) {
            c_hi = c;
            for (int64_t t = tid; t <= K; t += LZ_T) spl_hi[t] = spl[t];
        } else {
            c_lo = c;
        }
        first = false;
        __syncthreads();
    }
    if (tid == 0) *nprobes = stuck ? -1 : probes;
