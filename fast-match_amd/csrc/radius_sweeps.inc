// The four threshold sweeps of K10 (radius.hip), included twice: R_SWEEP_MASKED false gives radius_{i8,f16,wide,ham}_kernel, the
// unmasked sweeps -- every `if constexpr (MASKED)` below is discarded and they are the kernels they were before masks existed --
// and R_SWEEP_MASKED true gives rmask_{i8,f16,wide,ham}_kernel, the sweeps of the masked entry points (r_mask_word, radius.hip).
// No include guard: R_SWEEP_KERNEL(route) names the kernel.
template <bool FILL>
__global__ __launch_bounds__(256)
void R_SWEEP_KERNEL(i8)(RSweep p)
{
    constexpr bool MASKED = R_SWEEP_MASKED;
    __shared__ __attribute__((aligned(16))) int8_t srow[kRStage * kRRowI8];
    __shared__ __attribute__((aligned(16))) int snorm[kRStage];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * kRQPerWG + wave * 16 * kRNB;
    v4i bq[kRNB][2];
    int qn[kRNB], lim[kRNB];
    unsigned count[kRNB];
#pragma unroll
    for (int b = 0; b < kRNB; ++b) {
        const int q = qw + 16 * b + j;
        const bool live = q < p.nq;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            bq[b][h] = live ? *(const v4i*)(p.qrows + (size_t)q * kDim + 64 * h + 16 * g) : v4i{0, 0, 0, 0};
        qn[b] = live ? p.qnorm[q] : 0;
        lim[b] = live ? p.lim[q] : -1;
        count[b] = 0;
    }
    const int t0 = blockIdx.y * p.per, t1 = min(p.nt, t0 + p.per);
    unsigned long long mnext[MASKED ? kRNB : 1];
    if constexpr (MASKED) {
#pragma unroll
        for (int b = 0; b < kRNB; ++b) mnext[b] = t0 < t1 ? r_mask_word(p, qw + 16 * b + j, t0) : 0ull;
    }
    for (int base = t0; base < t1; base += kRStage) {
        unsigned mbits[MASKED ? kRNB : 1];
        bool wave_on = true;
        if constexpr (MASKED) {             // this stage's bits; the next stage's words go out in front of this stage's copy
#pragma unroll
            for (int b = 0; b < kRNB; ++b) mbits[b] = r_word_bits(mnext[b], g);
            if (base + kRStage < t1) {
#pragma unroll
                for (int b = 0; b < kRNB; ++b) mnext[b] = r_mask_word(p, qw + 16 * b + j, base + kRStage);
            }
            wave_on = __any((mbits[0] | mbits[1] | mbits[2] | mbits[3]) != 0u);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {       // 64 rows x 8 pieces of 16 B (rows < n_pad: base % 64 == 0, n_pad % 128 == 0)
            const int piece = tid + 256 * i, r = piece >> 3, c = piece & 7;
            *(v4i*)(srow + r * kRRowI8 + 16 * c) = *(const v4i*)(p.trows + (size_t)(base + r) * kDim + 16 * c);
        }
        if (tid < kRStage) snorm[tid] = p.tnorm[base + tid];
        __syncthreads();
        // (both barriers of a stage are passed by every wave; a wave whose rows permit nothing in the stage skips what lies
        // between this one and the next stage's: the operand reads from LDS and the MFMAs)
        if (!wave_on) continue;
        v4i a[4][2], tn[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) a[tt][h] = *(const v4i*)(srow + (16 * tt + j) * kRRowI8 + 64 * h + 16 * g);
            tn[tt] = *(const v4i*)(snorm + 16 * tt + 4 * g);
        }
        const int rowlim = r_real_end(p, base, t1) - base - 4 * g;   // register r of tile tt is a real train row iff 16 tt + r < rowlim
#pragma unroll
        for (int b = 0; b < kRNB; ++b) {
            if constexpr (MASKED) { if (!__any(mbits[b] != 0u)) continue; }      // (wave-uniform: a block without a permitted pair)
            unsigned mask = 0;
            unsigned hi[16];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tt][0], bq[b][0], v4i{0, 0, 0, 0}, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tt][1], bq[b][1], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int d2 = qn[b] + tn[tt][r] - 2 * acc[r];
                    hi[4 * tt + r] = FILL ? sqrt_bits((unsigned)d2) : 0u;
                    mask |= (d2 <= lim[b] && 16 * tt + r < rowlim) ? (1u << (4 * tt + r)) : 0u;
                }
            }
            if (p.real) mask &= r_real_bits(p.real, base, g);         // (uniform branch; a gap row of a grown bank is no hit)
            if constexpr (MASKED) mask &= mbits[b];
            if constexpr (FILL) r_emit(p, mask, hi, qw + 16 * b + j, qw + 16 * b + j < p.nq, base, lane);
            else count[b] += __popc(mask);
        }
    }
    if constexpr (!FILL) {
#pragma unroll
        for (int b = 0; b < kRNB; ++b) {
            unsigned c = count[b];
            c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            const int q = qw + 16 * b + j;
            if (g == 0 && q < p.nq && c) atomicAdd(&p.cnt[q], c);
        }
    }
}

template <bool FILL>
__global__ __launch_bounds__(256)
void R_SWEEP_KERNEL(f16)(RSweep p)
{
    constexpr bool MASKED = R_SWEEP_MASKED;
    __shared__ __attribute__((aligned(16))) char srow[kRStage * kRRowH];
    __shared__ __attribute__((aligned(16))) float snorm[kRStage];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * kRQPerWG + wave * 16 * kRNB;
    const bool all = p.all != 0;
    rv8h bh[kRNB][4];
    float qn[kRNB], thr[kRNB];
    unsigned count[kRNB];
#pragma unroll
    for (int b = 0; b < kRNB; ++b) {
        const int q = qw + 16 * b + j;
        const bool live = q < p.nq;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const v4i h = (live && !all) ? *(const v4i*)(p.qrowsh + (size_t)q * kDim + 32 * s + 8 * g) : v4i{0, 0, 0, 0};
            bh[b][s] = __builtin_bit_cast(rv8h, h);
        }
        qn[b] = (live && !all) ? p.qnormf[q] * p.cq : 0.f;
        thr[b] = live ? p.thr[q] : -INFINITY;
        count[b] = 0;
    }
    unsigned hi[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) hi[c] = 0u;
    const int t0 = blockIdx.y * p.per, t1 = min(p.nt, t0 + p.per);
    unsigned long long mnext[MASKED ? kRNB : 1];
    if constexpr (MASKED) {
#pragma unroll
        for (int b = 0; b < kRNB; ++b) mnext[b] = t0 < t1 ? r_mask_word(p, qw + 16 * b + j, t0) : 0ull;
    }
    for (int base = t0; base < t1; base += kRStage) {
        unsigned mbits[MASKED ? kRNB : 1];
        bool on[MASKED ? kRNB : 1];
        bool wave_on = true;
        if constexpr (MASKED) {             // this stage's bits; the next stage's words go out in front of this stage's work
#pragma unroll
            for (int b = 0; b < kRNB; ++b) mbits[b] = r_word_bits(mnext[b], g);
            if (base + kRStage < t1) {
#pragma unroll
                for (int b = 0; b < kRNB; ++b) mnext[b] = r_mask_word(p, qw + 16 * b + j, base + kRStage);
            }
#pragma unroll
            for (int b = 0; b < kRNB; ++b) on[b] = __any(mbits[b] != 0u);     // (wave-uniform)
            wave_on = on[0] || on[1] || on[2] || on[3];
        }
        if (!all) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // 64 rows x 16 pieces of 16 B
                const int piece = tid + 256 * i, r = piece >> 4, c = piece & 15;
                *(v4i*)(srow + r * kRRowH + 16 * c) = *(const v4i*)(p.trowsh + (size_t)(base + r) * kDim + 8 * c);
            }
            if (tid < kRStage) snorm[tid] = p.tnormf[base + tid] * p.ct;
            __syncthreads();
        }
        if (!wave_on) continue;             // (behind the stage's barriers, which every wave passes, as in the integer sweep)
        const int rowlim = r_real_end(p, base, t1) - base - 4 * g;
        unsigned mask[kRNB];
#pragma unroll
        for (int b = 0; b < kRNB; ++b) mask[b] = 0;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            rv8h a[4];
            rv4f tn = rv4f{0.f, 0.f, 0.f, 0.f};
            if (!all) {
#pragma unroll
                for (int s = 0; s < 4; ++s) a[s] = __builtin_bit_cast(rv8h, *(const v4i*)(srow + (16 * tt + j) * kRRowH + 64 * s + 16 * g));
                tn = *(const rv4f*)(snorm + 16 * tt + 4 * g);
            }
#pragma unroll
            for (int b = 0; b < kRNB; ++b) {
                if constexpr (MASKED) { if (!on[b]) continue; }       // a block without a permitted pair in the stage
                rv4f acc = rv4f{0.f, 0.f, 0.f, 0.f};
                if (!all) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], bh[b][s], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float A = qn[b] + tn[r] - 2.f * acc[r];     // (all: 0, against a threshold of +-inf)
                    mask[b] |= (A <= thr[b] && 16 * tt + r < rowlim) ? (1u << (4 * tt + r)) : 0u;
                }
            }
        }
#pragma unroll
        for (int b = 0; b < kRNB; ++b) {
            const int q = qw + 16 * b + j;
            if constexpr (MASKED) mask[b] &= mbits[b];
            if constexpr (FILL) {
#pragma unroll
                for (int c = 0; c < 16; ++c) hi[c] = (unsigned)q;
                r_emit(p, mask[b], hi, q, q < p.nq, base, lane);
            } else {
                count[b] += __popc(mask[b]);
            }
        }
    }
    if constexpr (!FILL) {
#pragma unroll
        for (int b = 0; b < kRNB; ++b) {
            unsigned c = count[b];
            c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            const int q = qw + 16 * b + j;
            if (g == 0 && q < p.nq && c) atomicAdd(&p.cnt[q], c);
        }
    }
}

// Wide route (file comment): the query rows of a wave -- two blocks of 16 -- are the B operand, in registers for the whole
// sweep; the train rows' fp16 plane comes straight from memory, one 16-row tile ahead (no LDS, no barrier).  A stage is four
// tiles: the 16 candidates a lane has per block in 64 rows go through r_emit like the float32 route's.  Every tile of a stage
// is read, also behind the split's end: the stage ends inside the bank's padded rows (base % 64 == 0, n_pad % 128 == 0), and
// what lies behind t1 or behind a collection's real rows is masked by index.
template <bool FILL, int KS>
__global__ __launch_bounds__(256)
void R_SWEEP_KERNEL(wide)(RSweep p)
{
    constexpr bool MASKED = R_SWEEP_MASKED;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * kRWQPerWG + wave * 16 * kRWNB;
    const bool all = p.all != 0;
    rv8h bh[kRWNB][KS];
    float qn[kRWNB], thr[kRWNB];
    unsigned count[kRWNB];
#pragma unroll
    for (int b = 0; b < kRWNB; ++b) {
        const int q = qw + 16 * b + j;
        const bool live = q < p.nq;      // (a chunk may start on any row: the rows behind nq need not lie inside the bank)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const v4i h = (live && !all) ? *(const v4i*)(p.qrowsh + (size_t)q * kWideDim + 32 * s + 8 * g) : v4i{0, 0, 0, 0};
            bh[b][s] = __builtin_bit_cast(rv8h, h);
        }
        qn[b] = (live && !all) ? p.qnormf[q] * p.cq : 0.f;
        thr[b] = live ? p.thr[q] : -INFINITY;
        count[b] = 0;
    }
    unsigned hi[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) hi[c] = 0u;
    const int t0 = blockIdx.y * p.per, t1 = min(p.nt, t0 + p.per);
    rv8h an[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) an[s] = rv8h{0, 0, 0, 0, 0, 0, 0, 0};
    if (!all && t0 < t1) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
            an[s] = __builtin_bit_cast(rv8h, *(const v4i*)(p.trowsh + (size_t)(t0 + j) * kWideDim + 32 * s + 8 * g));
    }
    unsigned long long mnext[MASKED ? kRWNB : 1];
    if constexpr (MASKED) {
#pragma unroll
        for (int b = 0; b < kRWNB; ++b) mnext[b] = t0 < t1 ? r_mask_word(p, qw + 16 * b + j, t0) : 0ull;
    }
    for (int base = t0; base < t1; base += kRStage) {
        // (a masked stage without a permitted pair keeps the tile-ahead fetch going and skips the MFMAs and the epilogue, block by block)
        unsigned mbits[MASKED ? kRWNB : 1];
        bool on[MASKED ? kRWNB : 1];
        bool wave_on = true;
        if constexpr (MASKED) {             // this stage's bits; the next stage's words go out in front of this stage's work
#pragma unroll
            for (int b = 0; b < kRWNB; ++b) mbits[b] = r_word_bits(mnext[b], g);
            if (base + kRStage < t1) {
#pragma unroll
                for (int b = 0; b < kRWNB; ++b) mnext[b] = r_mask_word(p, qw + 16 * b + j, base + kRStage);
            }
#pragma unroll
            for (int b = 0; b < kRWNB; ++b) on[b] = __any(mbits[b] != 0u);     // (wave-uniform)
            wave_on = on[0] || on[1];
        }
        (void)wave_on;                      // (no stage-wide skip here: the fetch of the next tile goes on)
        const int rowlim = r_real_end(p, base, t1) - base - 4 * g;   // register r of tile tt is a real train row iff 16 tt + r < rowlim
        const bool more = base + kRStage < t1;
        unsigned mask[kRWNB];
#pragma unroll
        for (int b = 0; b < kRWNB; ++b) mask[b] = 0;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            rv8h a[KS];
            rv4f tn = rv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) a[s] = an[s];
            if (!all) {
                if (tt < 3 || more) {       // the next tile: of this stage, or the first of the next one
#pragma unroll
                    for (int s = 0; s < KS; ++s)
                        an[s] = __builtin_bit_cast(rv8h, *(const v4i*)(p.trowsh + (size_t)(base + 16 * (tt + 1) + j) * kWideDim + 32 * s + 8 * g));
                }
                tn = *(const rv4f*)(p.tnormf + base + 16 * tt + 4 * g) * p.ct;
            }
#pragma unroll
            for (int b = 0; b < kRWNB; ++b) {
                if constexpr (MASKED) { if (!on[b]) continue; }
                rv4f acc = rv4f{0.f, 0.f, 0.f, 0.f};
                if (!all) {
#pragma unroll
                    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], bh[b][s], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float A = qn[b] + tn[r] - 2.f * acc[r];     // (all: 0, against a threshold of +-inf)
                    mask[b] |= (A <= thr[b] && 16 * tt + r < rowlim) ? (1u << (4 * tt + r)) : 0u;
                }
            }
        }
#pragma unroll
        for (int b = 0; b < kRWNB; ++b) {
            const int q = qw + 16 * b + j;
            if constexpr (MASKED) mask[b] &= mbits[b];
            if constexpr (FILL) {
#pragma unroll
                for (int c = 0; c < 16; ++c) hi[c] = (unsigned)q;
                r_emit(p, mask[b], hi, q, q < p.nq, base, lane);
            } else {
                count[b] += __popc(mask[b]);
            }
        }
    }
    if constexpr (!FILL) {
#pragma unroll
        for (int b = 0; b < kRWNB; ++b) {
            unsigned c = count[b];
            c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            const int q = qw + 16 * b + j;
            if (g == 0 && q < p.nq && c) atomicAdd(&p.cnt[q], c);
        }
    }
}

// Hamming route (binary banks, K11's operands: hamming.hip): every bit is one FP4 value, +1 or -1, so the dot product of two
// encoded rows is W - 2 h, exact in the f32 accumulator; a hit is dot >= thr (ham_radius.h), h = (W - dot) / 2.  K11's loop:
// 128-row stages through two LDS buffers, the next stage prefetched into registers, one barrier per stage, row pitch RB + 16;
// the 64 query rows of a wave are the B operand, in registers for the whole sweep.  A split is whole stages (p.per rows).
// Padding rows are all-zero FP4 rows at dot = 0 -- h = W / 2, inside any r > W / 2 -- and are kept out by index: rows from
// `lim` on (the bank's nt, or the real rows of a collection's stage) never count; only a last, partial stage pays for the test.
// MASKED: a 128-row stage is two mask words per query row, one per `half`; the count pass collects the hit bits of a half as
// the fill pass does (the unmasked count pass keeps its plain counter), and both AND the words' bits in before they count or
// emit.  A half in which no row of the wave permits anything skips its operand reads from LDS and its MFMAs (no skip per block
// here: a branch round each block's MFMAs costs the fill sweep a wave per SIMD in registers); the stage's cooperative load, its
// store and its barrier are every wave's as before.
template <bool FILL, int KS>
__global__ __launch_bounds__(256)
void R_SWEEP_KERNEL(ham)(RSweep p)
{
    constexpr bool MASKED = R_SWEEP_MASKED;
    constexpr bool BITS = FILL || MASKED;   // the hits of a half as a bit mask (r_emit's layout)
    constexpr int RB = KS * 64;             // FP4 bytes per row
    constexpr int LS = RB + 16;             // LDS row pitch
    constexpr int PIECES = kStageRows * RB / 16 / 256;    // 16-byte pieces per thread per stage (2 KS)
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStageRows * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * kRQPerWG + wave * 16 * kRNB;
    const int nstages = (p.nt + kStageRows - 1) / kStageRows;
    const int st0 = blockIdx.y * (p.per / kStageRows), st1 = min(nstages, st0 + p.per / kStageRows);

    rv8i bop[kRNB][KS];
    float thr[kRNB];
    unsigned count[kRNB];
#pragma unroll
    for (int b = 0; b < kRNB; ++b) {
        const int q = qw + 16 * b + j;
        const bool live = q < p.nq;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i x = live ? *(const v4i*)(p.q4 + (size_t)q * RB + 64 * ks + 16 * g) : v4i{0, 0, 0, 0};
            bop[b][ks] = rv8i{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
        }
        thr[b] = live ? p.thr[q] : INFINITY;
        count[b] = 0;
    }

    v4i pre[PIECES];
    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i)      // (whole stages: st < nstages <= n_pad / 128)
            pre[i] = *(const v4i*)(p.t4 + ((size_t)st * kStageRows) * RB + (size_t)(tid + 256 * i) * 16);
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int pc = tid + 256 * i;
            *(v4i*)(&lds[buf][(pc / (RB / 16)) * LS + 16 * (pc % (RB / 16))]) = pre[i];
        }
    };
    unsigned long long mnext[MASKED ? kRNB : 1][2];
    if constexpr (MASKED) {
#pragma unroll
        for (int b = 0; b < kRNB; ++b)
#pragma unroll
            for (int half = 0; half < 2; ++half)
                mnext[b][half] = st0 < st1 ? r_mask_word(p, qw + 16 * b + j, st0 * kStageRows + 64 * half) : 0ull;
    }
    if (st0 < st1) { load(st0); store(0); }
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
        const int buf = (st - st0) & 1;
        const bool more = st + 1 < st1;
        unsigned mbits[MASKED ? kRNB : 1];           // the lane's 16 bits of half 0 | of half 1 << 16
        if constexpr (MASKED) {
#pragma unroll
            for (int b = 0; b < kRNB; ++b) mbits[b] = r_word_bits(mnext[b][0], g) | (r_word_bits(mnext[b][1], g) << 16);
            if (more) {                              // the next stage's words, beside its rows
#pragma unroll
                for (int b = 0; b < kRNB; ++b)
#pragma unroll
                    for (int half = 0; half < 2; ++half)
                        mnext[b][half] = r_mask_word(p, qw + 16 * b + j, (st + 1) * kStageRows + 64 * half);
            }
        }
        if (more) load(st + 1);
        const int sbase = st * kStageRows;
        const int lim = p.st_real ? sbase + p.st_real[st] : p.nt;       // (uniform: one table word per stage)
        const bool tail = sbase + kStageRows > lim;
        const int rowlim = lim - sbase - 4 * g;      // tail: register r of tile t is a real train row iff 16 t + r < rowlim
#pragma unroll
        for (int half = 0; half < 2; ++half) {       // r_emit takes the 16 candidates a lane has in 64 rows
            unsigned mask[kRNB];
            float dot[FILL ? kRNB : 1][16];
#pragma unroll
            for (int b = 0; b < kRNB; ++b) mask[b] = 0;
            unsigned mh[MASKED ? kRNB : 1];
            if constexpr (MASKED) {
#pragma unroll
                for (int b = 0; b < kRNB; ++b) mh[b] = (mbits[b] >> (16 * half)) & 0xFFFFu;
                if (!__any((mh[0] | mh[1] | mh[2] | mh[3]) != 0u)) continue;     // (wave-uniform; no barrier inside a half)
            }
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int t = 4 * half + tt;
                rv8i aop[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const v4i x = *(const v4i*)(&lds[buf][(16 * t + j) * LS + 64 * ks + 16 * g]);
                    aop[ks] = rv8i{x[0], x[1], x[2], x[3], 0, 0, 0, 0};
                }
#pragma unroll
                for (int b = 0; b < kRNB; ++b) {
                    rv4f acc = rv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aop[ks], bop[b][ks], acc, 4, 4, 0, 127, 0, 127);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        bool hit = acc[r] >= thr[b];
                        if (tail) hit = hit && 16 * t + r < rowlim;
                        if constexpr (BITS) mask[b] |= hit ? (1u << (4 * tt + r)) : 0u;
                        else count[b] += hit ? 1u : 0u;
                        if constexpr (FILL) dot[b][4 * tt + r] = acc[r];
                    }
                }
            }
            if constexpr (MASKED) {
#pragma unroll
                for (int b = 0; b < kRNB; ++b) {
                    mask[b] &= mh[b];
                    if constexpr (!FILL) count[b] += __popc(mask[b]);
                }
            }
            if constexpr (FILL) {
#pragma unroll
                for (int b = 0; b < kRNB; ++b) {
                    if (!__any(mask[b] != 0)) continue;
                    unsigned hi[16];
#pragma unroll
                    for (int c = 0; c < 16; ++c) hi[c] = __float_as_uint((float)((p.W - (int)dot[b][c]) >> 1));
                    r_emit(p, mask[b], hi, qw + 16 * b + j, qw + 16 * b + j < p.nq, sbase + 64 * half, lane);
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
    if constexpr (!FILL) {
#pragma unroll
        for (int b = 0; b < kRNB; ++b) {
            unsigned c = count[b];
            c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            const int q = qw + 16 * b + j;
            if (g == 0 && q < p.nq && c) atomicAdd(&p.cnt[q], c);
        }
    }
}
