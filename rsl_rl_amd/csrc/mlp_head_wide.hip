// The fused actor head for 17 to 32 actions: the last hidden layer, the output layer, the PPO loss and the output
// layer's backward in one launch on the tiled GEMM's kEpiBiasEluOut epilogue (mlp_gemm_x6.h), as mlp_heads.hip's heads
// for 5 to 16 actions.  A unit of its own: it instantiates the main loop for its four widths.
//   rslrl_actor_head_wide_fwd_bwd   actor: mu, the PPO loss and its statistics, d mu, dZ, [dW | db] partials
#include "actor_head_host.h"
#include "common.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

// the H half-tile stage of a wave row: [32 rows][256], float4 quads XOR-swizzled in their 8-quad group by row & 7
__device__ __forceinline__ int wide_stage_idx(int l, int quad) { return l * kBN + 4 * (quad ^ (l & 7)); }

// ---- The wide actor head: A = p.nout in [kActWideMinA, kActWideMaxA] = 17 .. 32 actions ------------------------------
// The same launch on the 32-wide padded problem.  At 32 outputs the reduction tiles of one half of the wave rows fill
// buffer 0, so the tile goes through the output layer, the loss and the backward in two half passes: half i = 1, then
// i = 0, of each wave row -- 64 rows a pass, hr = 32 wm + l (tile row 64 wm + 32 i + l).
// LDS: red [wm][wn][32 outputs][32 rows] = b0 [0, 32K) (the row index XORed with 8 ((o >> 2) & 3): the loss's reads
// of four actions per lane spread over the banks); the H half-tile stages = b0 / b1 [0, 32K) once red is read; the
// d mu half tile [64][32] = b1 [32K, 40K), its float4 quads XOR-swizzled by row & 7 (the dZ fragment reads walk rows
// at a stride of 32 floats); wstat [8 waves][36], folded [68], db [32] fp64 and the flag = b0 [32768, 35876); the side area
// (bias [256], then kActSideRows rows of 32 floats) = b0 [36864, 39424).
// Per pass:
//  1. H = ELU(acc[i] + b) in place, the output layer's partial tiles (the fused forward's MFMA epilogue: all 16
//     registers of the 32 x 32 tile) -> red; the row's loss inputs are requested.                         barrier
//  2. mu of row hr on lanes q = 0..7 of its octet, actions 4 q .. 4 q + 3 below A (the four wn partials in the fused
//     forward's order + the output bias: linear_fwd_out_ex's bits).                                        barrier
//  3. H of the half into the stages (acc[i] dies here); the loss of the row on its octet: ppo_loss_kernel's
//     expressions on the per-action constants of the side area; the log-prob is tree_sum<32>'s sum -- the lane's four
//     terms as a running sum, then an xor butterfly over the octet (two quad_perm steps and row_half_mirror; every
//     step a commutative add, so all eight lanes hold ppo_loss_kernel<32>'s bits) -> d mu half tile (a slot past A
//     works on action A - 1, adds to no sum, stores nothing to global memory and writes an exact +0), the wave's fp64
//     loss partials (the second pass adds to the first's).                                                  barrier
//  4. db: wave 0, lane (o, rows 32 part ..) in row order, in fp64 and kept in fp64 (below); dW: thread (column c,
//     action group ag of 16) walks column c of both stages' 64 rows with the d mu row broadcast from LDS -- 16
//     accumulators, kept over both passes, no cross-thread sum.                                           barrier
//  5. dZ = (d mu W_out) * ELU'(H): two 16-deep x6 MFMA k steps per 32 x 32 block on the W_out^T image (zero from
//     k = A on) and the split d mu rows; H comes back from the wave's own stage region and dZ leaves through it as
//     whole lines at row stride N.  A dead wave column (NW < 4) skips 1 (zeros into red), its stage, dW and dZ.  barrier
// Then the per-tile [dW | db | 0] row and two grid folds of fp64 columns (fold_grid_partials<36>, <32>): the loss's
// 4 + A, then the tiles' db.  A tile's db rounded to fp32 in its partial row costs half an ulp per tile, which is more
// than torch.sum's error on the same d mu; so every tile writes zeros into its row's db slots, and the block that
// finishes the second fold writes the whole db -- an fp64 sum in a fixed order, rounded once -- into the db slots of its
// own row.  The fold of the partial rows adds that one value to zeros: exact, whichever tile held it.
__device__ __forceinline__ int wide_red_idx(int o, int r) { return o * 32 + (r ^ (((o >> 2) & 3) << 3)); }
__device__ __forceinline__ int wide_dmu_idx(int r, int quad) { return r * kActWideMaxA + 4 * (quad ^ (r & 7)); }

template <int NW>
__device__ __forceinline__ void actor_head_wide_epilogue(const GemmParams& p, const ActorParams& ap,
                                                         f32x16 (&acc)[2][2], char* lds0, char* lds1, const float* xsb,
                                                         int wm, int wn, int lane, int wave, int64_t row0) {
    constexpr int kW = kActWideMaxA;      // the padded width: side-row stride, d mu columns
    constexpr int kRed = kW * 32;         // floats of one (wm, wn) reduction tile
    constexpr int kWs = kActWideCols;     // stride of a wave's loss partials
    constexpr int kN = 64 * NW;           // = p.N: row stride of dz and of the dW partial rows
    constexpr int kDwA = 16;              // actions per dW thread group
    static_assert(NW >= 1 && NW <= 4, "wide actor head: N = 64, 128, 192 or 256");
    static_assert(2 * 4 * kRed * 4 <= 32768, "wide actor head: red below the loss partials");
    static_assert(64 * kW * 4 <= 40960 - 32768, "wide actor head: the d mu half tile behind buffer 1's stage");
    static_assert(32768 + kActWideStatBytes <= 36864, "wide actor head: loss partials below the side area");
    static_assert(36864 + 4 * (kBN + kActSideRows * kW) <= 40960, "wide actor head: side area inside buffer 0");
    static_assert(2 * kDwA == kW && kThreads == 2 * kBN, "wide actor head: two dW action groups over 256 columns");
    const int A = p.nout;                  // wave-uniform
    const bool live = NW == 4 || wn < NW;  // wave-uniform
    const int cols = 4 + A;  // the loss's fold: surrogate, value, entropy, KL, d sigma [A]
    const int l32 = lane & 31, h = lane >> 5;
    const int t = threadIdx.x;
    float* red = reinterpret_cast<float*>(lds0);
    float* dmu = reinterpret_cast<float*>(lds1 + 32768);
    double* wstat = reinterpret_cast<double*>(lds0 + 32768);  // [8 waves][kWs]
    double* folded = wstat + 8 * kWs;                         // [kActWideFoldCols]: the loss's kWs, then db's kW
    double* dbl = folded + kActWideFoldCols;                  // [kW] the tile's db
    int* flag = reinterpret_cast<int*>(dbl + kW);
    float* const stg = reinterpret_cast<float*>(wm ? lds1 : lds0);  // this wave row's half-tile H stage
    // ---- 0. the loss's per-action constants, once per tile, on 32 lanes of the last wave (a slot past A: of sigma 1)
    if (t >= kThreads - kWave && t < kThreads - kWave + kW) {
        float* side = const_cast<float*>(xsb) + kBN;
        const int a = t - (kThreads - kWave);
        const bool in = a < A;
        const float sv = side[kSideSigma * kW + a], o0 = side[kSideOldSigma * kW + a];
        const SigmaConsts c = sigma_consts(in ? sv : 1.0f);
        const KlFastConsts f = kl_fast_consts(c.s, in ? o0 : 1.0f, ap.kl_fast);
        side[kSideSigma * kW + a] = c.s;
        side[kSideLs * kW + a] = c.ls;
        side[kSideInvDen * kW + a] = c.inv_den;
        side[kSideInvS * kW + a] = c.inv_s;
        side[kSideInvS3 * kW + a] = c.inv_s3;
        side[kSideKlOs * kW + a] = f.os;
        side[kSideKlT1 * kW + a] = f.t1;
        side[kSideKlD * kW + a] = f.D;
        side[kSideKlRD * kW + a] = f.rD;
        float ent = 0.0f;  // the entropy of a row: the A actions in order
#pragma unroll
        for (int b = 0; b < kW; ++b) {
            const float lb = __shfl(c.ls, b, kWave);  // lanes 0..31 of this wave are all here
            if (b < A) ent = __fadd_rn(ent, entropy_term(lb));
        }
        if (a == 0) side[kSideEnt * kW] = ent;
    }
    const float* xact = xsb + kBN;
    auto cst = [&](int r, int a) { return xact[r * kW + a]; };
    const uint4* oimg = p.oimg + wn * (2 * 2 * 3 * 64);
    // the loss: row hr of the half on lanes q = 0..7, actions a0 .. a0 + 3 below A
    const int hr = t >> 3, q = t & 7, a0 = 4 * q;
    bool ok[4];
    int ak[4];  // a masked slot works on the last action's data (finite, in bounds) and stores and adds nothing
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = a0 + k < A;
        ak[k] = min(a0 + k, A - 1);
    }
    // the backward: dW column c, actions kDwA ag .. (wave-uniform ag; column c belongs to wave column c >> 6 = wn)
    const int c = t & (kBN - 1), ag = t >> 8;
    float wacc[kDwA];  // (zeroed where the first pass starts its dW: not live through that pass's output layer and loss)
    double dbs = 0.0;  // wave 0: db of column lane & 31 (both halves of the lanes hold the sum)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int i = 1 - pass;
        // ---- 1. H of half i and the output layer's partials
        {
            f32x16 oacc = f32x16{};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!live) continue;
                const int cb = wn * 64 + j * 32 + 4 * h;
                float v[16];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 b4 = *reinterpret_cast<const float4*>(xsb + cb + 8 * g);
                    float tt[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    tt[0] += b4.x;
                    tt[1] += b4.y;
                    tt[2] += b4.z;
                    tt[3] += b4.w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float n = elu_neg(fminf(tt[e], 0.f));
                        v[4 * g + e] = tt[e] > 0.f ? tt[e] : n;
                        acc[i][j][4 * g + e] = v[4 * g + e];
                    }
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 vb[3], wa[3];
                    uint2 lo[3], hi[3];
                    split4(make_float4(v[8 * s2], v[8 * s2 + 1], v[8 * s2 + 2], v[8 * s2 + 3]), lo[0], lo[1], lo[2]);
                    split4(make_float4(v[8 * s2 + 4], v[8 * s2 + 5], v[8 * s2 + 6], v[8 * s2 + 7]), hi[0], hi[1], hi[2]);
#pragma unroll
                    for (int qq = 0; qq < 3; ++qq) {
                        vb[qq] = __builtin_bit_cast(bf16x8, make_uint4(lo[qq].x, lo[qq].y, hi[qq].x, hi[qq].y));
                        wa[qq] = __builtin_bit_cast(bf16x8, oimg[((j * 2 + s2) * 3 + qq) * 64 + lane]);
                    }
                    oacc = mfma_x6(wa, vb, oacc);
                    __builtin_amdgcn_sched_barrier(0);  // one k step at a time: its planes die before the next split
                }
            }
            float* rd = red + (wm * 4 + wn) * kRed;
#pragma unroll
            for (int r = 0; r < 16; ++r) rd[wide_red_idx((r & 3) + 8 * (r >> 2) + 4 * h, l32)] = oacc[r];
        }
        // the row's loss inputs: wave-uniform tile bases and 32-bit element offsets
        const int rl = (hr >> 5) * 64 + i * 32 + (hr & 31);
        const int64_t row = row0 + rl;
        const int64_t tile0 = row0 * A;
        const uint32_t e0 = static_cast<uint32_t>(rl * A);
        float x[4], om[4], os[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = (ap.actions + tile0)[e0 + ak[k]];
            om[k] = (ap.old_mu + tile0)[e0 + ak[k]];
            os[k] = (ap.old_sigma + tile0)[e0 + ak[k]];
        }
        const float old_logp = ap.old_logp[row], adv = ap.adv[row], V = ap.values[row], tv = ap.target_values[row],
                    R = ap.returns[row];
        __syncthreads();  // red (and, in the first pass, the per-action constants) complete
        // ---- 2. mu
        float mu[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* b = red + (hr >> 5) * 4 * kRed + wide_red_idx(ak[k], hr & 31);
            const float sum = ((b[0] + b[kRed]) + b[2 * kRed]) + b[3 * kRed];
            mu[k] = sum + xact[ak[k]];
            if (ok[k]) (p.y + tile0)[e0 + ak[k]] = mu[k];
        }
        __syncthreads();  // red read: buffer 0 takes the H stage
        // ---- 3. the H stage of the half, then the loss of the row on its octet
        if (live) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 hv = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(stg + wide_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h)) = hv;
                }
        }
        float d[4], lsum = 0.0f, klpart = 0.0f;
        bool kl_slow = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = x[k] - mu[k];
            const float term = logp_term(d[k], cst(kSideInvDen, ak[k]), cst(kSideLs, ak[k]));
            // tree_sum: a running sum inside the lane's block of four, entries from A on count as 0
            lsum = k == 0 ? (ok[0] ? term : 0.0f) : __fadd_rn(lsum, ok[k] ? term : 0.0f);
            const KlFastConsts kf = {cst(kSideKlOs, ak[k]), cst(kSideKlT1, ak[k]), cst(kSideKlD, ak[k]),
                                     cst(kSideKlRD, ak[k])};
            bool slow = false;
            const float kt = kl_term_fast(kf, os[k], mu[k], om[k], slow);
            if (ok[k]) {
                klpart = __fadd_rn(klpart, kt);
                kl_slow |= slow;
            }
        }
        if (ap.compute_kl && kl_slow) {  // the reference's exact expression for every element of this lane (rare)
            klpart = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float kt = kl_term_exact(cst(kSideSigma, ak[k]), os[k], mu[k], om[k]);
                if (ok[k]) klpart = __fadd_rn(klpart, kt);
            }
        }
        const float ent_shared = cst(kSideEnt, 0);
        const float logp = octet_sum(lsum);  // then the tree over the eight blocks, strides 1, 2, 4
        float gj, vterm;
        const float sterm = surrogate(logp, old_logp, adv, ap.ratio_lo, ap.ratio_hi, ap.g_surr, gj);
        // the value loss term only: its gradient is the critic head's, so g_value is unused
        (void)value_loss(V, tv, R, ap.clipped_value, ap.clip, 0.0f, vterm);
        float gsg[4], gmv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gm, gs;
            normal_grads(d[k], cst(kSideInvDen, ak[k]), cst(kSideInvS, ak[k]), cst(kSideInvS3, ak[k]), gj, ap.g_ent, gm,
                         gs);
            gsg[k] = ok[k] ? gs : 0.0f;
            gmv[k] = ok[k] ? gm : 0.0f;
            if (ap.grad_mu && ok[k]) (ap.grad_mu + tile0)[e0 + ak[k]] = gm;
        }
        *reinterpret_cast<float4*>(dmu + wide_dmu_idx(hr, q)) = make_float4(gmv[0], gmv[1], gmv[2], gmv[3]);
        {
            const double s_surr = wave_sum(static_cast<double>(q == 0 ? sterm : 0.0f));
            const double s_val = wave_sum(static_cast<double>(q == 0 ? vterm : 0.0f));
            const double s_ent = wave_sum(static_cast<double>(q == 0 ? ent_shared : 0.0f));
            const double s_kl = wave_sum(static_cast<double>(ap.compute_kl ? klpart : 0.0f));
            double* ws = wstat + wave * kWs;
            if (lane == 0) {  // (the same lanes write in both passes: the second adds to the first's sums)
                ws[0] = pass ? ws[0] + s_surr : s_surr;
                ws[1] = pass ? ws[1] + s_val : s_val;
                ws[2] = pass ? ws[2] + s_ent : s_ent;
                ws[3] = pass ? ws[3] + s_kl : s_kl;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double v = static_cast<double>(gsg[k]);
#pragma unroll
                for (int off = 8; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
                if (lane < 8 && 4 * lane + k < A) ws[4 + 4 * lane + k] = pass ? ws[4 + 4 * lane + k] + v : v;
            }
        }
        __syncthreads();  // the d mu half tile and the H stages complete
        // ---- 4. db and dW of the half
        if (wave == 0) {  // lane (o, part) adds rows 32 part .. 32 part + 31 of column o in order, then the two parts
            const int o = lane & 31, part = lane >> 5;
            double s = 0.0;  // fp64: the tile's db is rounded once, when the partial row is written
#pragma unroll 8
            for (int r = 32 * part; r < 32 * part + 32; ++r)
                s += static_cast<double>(dmu[wide_dmu_idx(r, o >> 2) + (o & 3)]);
            s += __shfl_xor(s, 32, kWave);
            dbs = pass ? dbs + s : s;
        }
        if (pass == 0)
#pragma unroll
            for (int o = 0; o < kDwA; ++o) wacc[o] = 0.f;
        if (live) {  // 4 broadcast d mu reads + 1 H read per 16 FMAs
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                const float* sb = reinterpret_cast<const float*>(rh ? lds1 : lds0);
#pragma unroll 4
                for (int l = 0; l < 32; ++l) {
                    const float hv = sb[wide_stage_idx(l, c >> 2) + (c & 3)];
#pragma unroll
                    for (int g = 0; g < kDwA / 4; ++g) {
                        const float4 d4 = *reinterpret_cast<const float4*>(dmu + wide_dmu_idx(rh * 32 + l, ag * 4 + g));
                        wacc[4 * g] = fmaf(d4.x, hv, wacc[4 * g]);
                        wacc[4 * g + 1] = fmaf(d4.y, hv, wacc[4 * g + 1]);
                        wacc[4 * g + 2] = fmaf(d4.z, hv, wacc[4 * g + 2]);
                        wacc[4 * g + 3] = fmaf(d4.w, hv, wacc[4 * g + 3]);
                    }
                }
            }
        }
        __syncthreads();  // every wave's reads of the stages done: dZ replaces H in place
        // ---- 5. dZ of the wave's two 32 x 32 blocks of the half
        if (live) {
            bf16x8 vb[2][3];  // the split d mu rows: k step s holds actions 16 s + 8 h .. + 7 of row 32 wm + l32
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int r = wm * 32 + l32;
                const float4 v0 = *reinterpret_cast<const float4*>(dmu + wide_dmu_idx(r, 4 * s + 2 * h));
                const float4 v1 = *reinterpret_cast<const float4*>(dmu + wide_dmu_idx(r, 4 * s + 2 * h + 1));
                uint2 lo[3], hi[3];
                split4(v0, lo[0], lo[1], lo[2]);
                split4(v1, hi[0], hi[1], hi[2]);
#pragma unroll
                for (int qq = 0; qq < 3; ++qq)
                    vb[s][qq] = __builtin_bit_cast(bf16x8, make_uint4(lo[qq].x, lo[qq].y, hi[qq].x, hi[qq].y));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x16 dacc = f32x16{};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8 wa[3];
#pragma unroll
                    for (int qq = 0; qq < 3; ++qq)
                        wa[qq] = read_frag<bf16x8>(reinterpret_cast<const char*>(ap.w_t_img) + s * kX6ChunkB +
                                                       qq * kX6PlaneB,
                                                   wn * 64 + j * 32 + l32, h);
                    dacc = mfma_x6(wa, vb[s], dacc);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float* sp = stg + wide_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h);
                    const f32x4 h4 = *reinterpret_cast<const f32x4*>(sp);
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = dacc[4 * g + e], hh = h4[e];
                        o[e] = hh > 0.f ? z : z * (hh + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
                    }
                    *reinterpret_cast<f32x4*>(sp) = o;
                }
                __builtin_amdgcn_wave_barrier();  // one wave's LDS accesses execute in order
                float* ct = p.c + (row0 + wm * 64 + i * 32) * kN + (wn * 64 + j * 32);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sr = 8 * k + (lane >> 3), cq = lane & 7;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(stg + wide_stage_idx(sr, wn * 16 + j * 8 + cq));
                    f32x4* dst = reinterpret_cast<f32x4*>(ct + static_cast<uint32_t>(sr * kN + 4 * cq));
                    if (p.nt) __builtin_nontemporal_store(v, dst);
                    else *dst = v;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();  // the stages and the d mu half tile are free: the next pass's red, the fold's flag
    }
    // ---- per-tile partials: [dW (A x N) | db | 0], then the loss terms over the grid
    float* wp = ap.wpart + static_cast<int64_t>(blockIdx.x) * act_tile_floats(A, kN);
    if (live)
#pragma unroll
        for (int o = 0; o < kDwA; ++o)
            if (kDwA * ag + o < A) wp[(kDwA * ag + o) * kN + c] = wacc[o];
    if (wave == 0) {  // db goes through the grid fold: the row's db slots and padding are zeros (but see below)
        if (lane < ((A + 3) & ~3)) wp[A * kN + lane] = 0.f;
        if (lane < kW) dbl[lane] = dbs;
    }
    __syncthreads();
    double v = 0.0;
    if (t < cols) {
        v = wstat[t];
#pragma unroll
        for (int w = 1; w < 8; ++w) v += wstat[w * kWs + t];
    }
    // two grid folds, each of at most 36 columns (one of 68 put scratch accesses into the main loop): the loss's
    // columns, then db on the second half of the tickets and behind the first fold's partials.  Groups of 64 tiles up
    // to 4096 tiles, of 128 above.
    const int nb = static_cast<int>(gridDim.x);
    const bool big = nb > kFoldGroup * kFoldGroup;
    const bool folded_ok = big ? fold_grid_partials<kWs, 2 * kFoldGroup>(ap.partials, ap.tickets, nb, cols, v, folded, flag)
                               : fold_grid_partials<kWs>(ap.partials, ap.tickets, nb, cols, v, folded, flag);
    if (folded_ok) {
        if (t == 0) {
            const double Bd = static_cast<double>(p.M);
            float* stats = ap.stats;
            stats[1] = static_cast<float>(folded[0] / Bd);
            stats[2] = static_cast<float>(folded[1] / Bd);
            stats[3] = static_cast<float>(folded[2] / Bd);
            stats[4] = static_cast<float>(folded[3] / Bd);
            stats[0] = __fsub_rn(__fadd_rn(stats[1], __fmul_rn(ap.value_loss_coef, stats[2])),
                                 __fmul_rn(ap.entropy_coef, stats[3]));
            stats[5] = 0.0f;
            stats[6] = 0.0f;
            stats[7] = 0.0f;
            __hip_atomic_store(ap.tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered)
        }
        if (t < A) ap.grad_sigma[t] = static_cast<float>(folded[4 + t]);
    }
    const int ng = (nb + kFoldGroup - 1) / kFoldGroup;  // >= the groups of 128: the first fold's partials end before
    double* part2 = ap.partials + static_cast<int64_t>(kWs) * (nb + ng);
    unsigned* tick2 = ap.tickets + kActWideTicketWords;
    double* folded2 = folded + kWs;  // [kW]
    const double v2 = t < A ? dbl[t] : 0.0;
    const bool db_ok = big ? fold_grid_partials<kW, 2 * kFoldGroup>(part2, tick2, nb, A, v2, folded2, flag)
                           : fold_grid_partials<kW>(part2, tick2, nb, A, v2, folded2, flag);
    if (db_ok) {
        if (t == 0) __hip_atomic_store(tick2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
        // the whole db, in this tile's row (wave 0's lanes: behind their own zero stores to the same words)
        if (t < A) wp[A * kN + t] = static_cast<float>(folded2[t]);
    }
}

// The actor head for p.nout = 17 .. 32 actions (rslrl_actor_head_wide_fwd_bwd; actor_head_wide_epilogue): a last hidden
// layer of N = 64 NW columns, 256 included, full 128-row tiles, x6.
template <int NW>
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_actor_head_wide_kernel(GemmParams p,
                                                                                const uint4* __restrict__ bimg,
                                                                                ActorParams ap) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    mlp_gemm_x6_body<kEpiBiasEluOut, true, 4, 3, true, 0, kHeadActorWide, NW>(p, bimg, lds_b0, lds_b1, &ap);
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

// The actor head for 17 to 32 actions (include/rslrl_amd.h): the same argument structs, a last hidden layer of 64, 128,
// 192 or 256 columns.  Every other shape returns RSLRL_E_UNSUPPORTED before anything is launched.  The workspace holds
// the fold's tickets and 4 + 2 x 32 fp64 partial columns per tile and per fold group.
extern "C" size_t rslrl_actor_head_wide_workspace_bytes(int64_t M) {
    const int64_t tiles = ceil_div(M > 0 ? M : 0, kBM);
    const int64_t groups = ceil_div(tiles, kFoldGroup);  // >= the groups of 128 a larger grid folds in
    return 1024 + sizeof(double) * static_cast<size_t>(kActWideFoldCols * (tiles + groups));
}

extern "C" int rslrl_actor_head_wide_fwd_bwd(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h,
                                             void* workspace, size_t workspace_bytes, rslrl_stream_t stream) {
    if (!a || !h || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    const int nw = a->N == kBN ? 4 : narrow_wave_cols(a->N);
    const int A = a->nout;
    if (a->arith != RSLRL_ARITH_X6 || !nw || a->K != 16 * kKC || A < kActWideMinA || A > kActWideMaxA)
        return RSLRL_E_UNSUPPORTED;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    const int64_t tiles = ceil_div(a->M, kBM);
    if (h->num_actions != A || a->M % kBM != 0 || a->M < 1 || !p.deep || tiles > int64_t{2 * kFoldGroup} * kFoldGroup)
        return RSLRL_E_UNSUPPORTED;
    ActorParams ap{};
    const int prc = actor_head_params(a, h, workspace, workspace_bytes, ap, rslrl_actor_head_wide_workspace_bytes(a->M),
                                      kl_fast_enabled());
    if (prc) return prc;
    const dim3 g(static_cast<unsigned>(tiles)), b(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint4* img = static_cast<const uint4*>(a->bimage);
    if (nw == 1) hipLaunchKernelGGL(mlp_gemm_x6_actor_head_wide_kernel<1>, g, b, 0, st, p, img, ap);
    else if (nw == 2) hipLaunchKernelGGL(mlp_gemm_x6_actor_head_wide_kernel<2>, g, b, 0, st, p, img, ap);
    else if (nw == 3) hipLaunchKernelGGL(mlp_gemm_x6_actor_head_wide_kernel<3>, g, b, 0, st, p, img, ap);
    else hipLaunchKernelGGL(mlp_gemm_x6_actor_head_wide_kernel<4>, g, b, 0, st, p, img, ap);
    return launch_status();
}
