// Everything that runs on the tiled GEMM's fused "last hidden layer + output layer" epilogue (mlp_gemm_x6.h,
// kEpiBiasEluOut): the plain forward RSLRL_LINEAR_FWD_OUT with its pair form, and the PPO update's fused heads -- one
// launch per network for the last hidden layer, the output layer, the loss term and the output layer's backward.
// (One unit: these kernels share one instantiation of the main loop.)
//   rslrl_value_head_fwd_bwd   critic: value head, d(value loss)/dV, dZ of the last hidden layer, [dW | db] partials
//                              (the epilogue is mlp_gemm_x6_body's HEAD = 1 branch; by default the streaming form,
//                              mlp_fwd_stream.hip, runs instead)
//   rslrl_actor_head_fwd_bwd   actor: mu, the PPO loss and its statistics, d mu, dZ, [dW | db] partials
//                              (actor_head_epilogue below: 12 actions; actor_head_any_epilogue<APL>: every other
//                              count from 5 to 16)
//   rslrl_value_head_fwd_bwd_n, rslrl_actor_head_fwd_bwd_n
//                              the same two launches for a last hidden layer of 64, 128 or 192 columns (NW = 1..3 live
//                              wave columns of the 256-column tile; the tiled kernels only)
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "fwd_stream.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

// ---- The actor head: last hidden layer + output layer + PPO loss + output-layer backward (one 128-row tile) ----------
// Called after the main loop of a full x6 C^T tile (acc: lane (l32, h) holds row l32 of block i, columns (r & 3) +
// 8 (r >> 2) + 4 h of block j).  Phases (LDS: buffer 0 = b0, buffer 1 = b1, 40 KiB each):
//  1. H = ELU(acc + b) in place; the output layer's partial tiles (x6 MFMA, the fused forward's epilogue: the same
//     bits) -> red [wm][wn][i][12][32] (b0 [0, 24K)).
//  2. mu of row t >> 2, actions 3 (t & 3) .. +2 (the wn partials added in the fused forward's order), then the loss of
//     the row on its quad of lanes: ppo_loss_quad_kernel's calls of ppo_loss_common.h (shared std; same d mu bits)
//     -> d mu tile [128][16] (b1 [32K, 40K), columns 12..15 zero) and per-wave fp64 loss partials (b0 [32K, 33K)).  The i = 1
//     half of H waits in LDS meanwhile (32 registers fewer through the loss).
//  3. per half i (1, then 0): H staged as [32 rows][256] per wave row wm (b0 / b1 [0, 32K), float4 quads XOR-swizzled
//     in their 8-quad group by row & 7); dW[o][c] += d mu[r][o] H[r][c] over the half's 64 rows, thread (c, o half)
//     with 6 accumulators; then dZ = (d mu W_out) * ELU'(H): x6 MFMA of the W_out^T image (A) and the split d mu
//     rows (B) gives the C^T layout of acc, ELU' from H, and the result leaves in place through the stage as
//     whole-line stores.
//  4. per-tile [dW | db] partials; loss partials folded over the grid (fold_grid_partials) -> stats, d sigma.
__device__ __forceinline__ int act_stage_idx(int l, int quad) { return l * kBN + 4 * (quad ^ (l & 7)); }

__device__ __forceinline__ void actor_head_epilogue(const GemmParams& p, const ActorParams& ap, f32x16 (&acc)[2][2],
                                                    char* lds0, char* lds1, const float* xsb, int wm, int wn, int lane,
                                                    int wave, int64_t row0) {
    const int l32 = lane & 31, h = lane >> 5;
    const int t = threadIdx.x;
    float* red = reinterpret_cast<float*>(lds0);
    float* dmu = reinterpret_cast<float*>(lds1 + 32768);
    double* wstat = reinterpret_cast<double*>(lds0 + 32768);  // [8 waves][kActCols]
    double* folded = wstat + 8 * kActCols;                    // [kActCols]
    int* flag = reinterpret_cast<int*>(folded + kActCols);
    float* const stg = reinterpret_cast<float*>(wm ? lds1 : lds0);  // this wave row's half-tile H stage
    // ---- 1. H and the output layer's partials
    const uint4* oimg = p.oimg + wn * (2 * 2 * 3 * 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        f32x16 oacc = f32x16{};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
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
                for (int q = 0; q < 3; ++q) {
                    vb[q] = __builtin_bit_cast(bf16x8, make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y));
                    wa[q] = __builtin_bit_cast(bf16x8, oimg[((j * 2 + s2) * 3 + q) * 64 + lane]);
                }
                oacc = mfma_x6(wa, vb, oacc);
                __builtin_amdgcn_sched_barrier(0);  // one k step at a time: its planes die before the next split
            }
        }
        float* rd = red + ((wm * 4 + wn) * 2 + i) * (kActA * 32);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (o < kActA) rd[o * 32 + l32] = oacc[r];
        }
    }
    // ---- 2. mu and the loss of row rl on lanes q = 0..3 (actions a0 .. a0 + 2)
    const int rl = t >> 2, q = t & 3, a0 = 3 * q;
    const int64_t row = row0 + rl;
    const float* xact = xsb + kBN;  // [obias | sigma | old_sigma of sample 0] x 12 (prologue)
    __syncthreads();  // red complete
    float mu[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* b = red + ((rl >> 6) * 4 * 2 + ((rl & 63) >> 5)) * (kActA * 32) + (a0 + k) * 32 + (rl & 31);
        const float sum = ((b[0] + b[2 * kActA * 32]) + b[4 * kActA * 32]) + b[6 * kActA * 32];
        mu[k] = sum + xact[a0 + k];
        p.y[row * kActA + a0 + k] = mu[k];
    }
    float x[3], om[3], os[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = ap.actions[row * kActA + a0 + k];
        om[k] = ap.old_mu[row * kActA + a0 + k];
        os[k] = ap.old_sigma[row * kActA + a0 + k];
    }
    const float old_logp = ap.old_logp[row], adv = ap.adv[row], V = ap.values[row], tv = ap.target_values[row],
                R = ap.returns[row];
    __syncthreads();  // red read: buffer 0 takes the H stage
    auto stage_half = [&](int i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 hv = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                *reinterpret_cast<f32x4*>(stg + act_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h)) = hv;
            }
    };
    stage_half(1);
    // the loss of the row on its quad, ppo_loss_quad_kernel's sequence of ppo_loss_common.h calls (SHARED = true)
    SigmaConsts cs[3];
    KlFastConsts kf[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cs[k] = sigma_consts(xact[kActA + a0 + k]);
        kf[k] = kl_fast_consts(cs[k].s, xact[2 * kActA + a0 + k], ap.kl_fast);
    }
    float ent_shared = 0.0f;  // sum over the 12 actions in order (the quad's lanes hold 3 each)
#pragma unroll
    for (int a = 0; a < kActA; ++a)
        ent_shared = __fadd_rn(ent_shared, entropy_term(__shfl(cs[a % 3].ls, (lane & ~3) + a / 3, kWave)));
    float d[3], lpart = 0.0f, klpart = 0.0f;
    bool kl_slow = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = x[k] - mu[k];
        lpart += logp_term(d[k], cs[k].inv_den, cs[k].ls);
        klpart = __fadd_rn(klpart, kl_term_fast(kf[k], os[k], mu[k], om[k], kl_slow));
    }
    if (ap.compute_kl && kl_slow) {  // the reference's exact expression for every element of this lane (rare)
        klpart = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) klpart = __fadd_rn(klpart, kl_term_exact(cs[k].s, os[k], mu[k], om[k]));
    }
    float gj, vterm;
    const float sterm = surrogate(quad_sum(lpart), old_logp, adv, ap.ratio_lo, ap.ratio_hi, ap.g_surr, gj);
    // the value loss term only: its gradient is the critic head's (rslrl_value_head_fwd_bwd), so g_value is unused
    (void)value_loss(V, tv, R, ap.clipped_value, ap.clip, 0.0f, vterm);
    float gsg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float gm;
        normal_grads(d[k], cs[k].inv_den, cs[k].inv_s, cs[k].inv_s3, gj, ap.g_ent, gm, gsg[k]);
        dmu[rl * 16 + a0 + k] = gm;
        if (ap.grad_mu) ap.grad_mu[row * kActA + a0 + k] = gm;
    }
    if (q == 3) *reinterpret_cast<float4*>(dmu + rl * 16 + kActA) = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        const double s_surr = wave_sum(static_cast<double>(q == 0 ? sterm : 0.0f));
        const double s_val = wave_sum(static_cast<double>(q == 0 ? vterm : 0.0f));
        const double s_ent = wave_sum(static_cast<double>(q == 0 ? ent_shared : 0.0f));
        const double s_kl = wave_sum(static_cast<double>(ap.compute_kl ? klpart : 0.0f));
        if (lane == 0) {
            wstat[wave * kActCols + 0] = s_surr;
            wstat[wave * kActCols + 1] = s_val;
            wstat[wave * kActCols + 2] = s_ent;
            wstat[wave * kActCols + 3] = s_kl;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double v = static_cast<double>(gsg[k]);
#pragma unroll
            for (int off = 4; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
            if (lane < 4) wstat[wave * kActCols + 4 + 3 * lane + k] = v;
        }
    }
    __syncthreads();  // the d mu tile and the i = 1 stage complete
    // ---- 3. output-layer backward, half i = 1 (staged) then i = 0 (registers)
    float* wp = ap.wpart + static_cast<int64_t>(blockIdx.x) * kActTileFloats;
    if (wave == 0) {  // db = column sums of d mu: lane (o, quarter) adds its 32 rows in order, then the quarters
        const int o = lane & 15, part = lane >> 4;
        float s = 0.f;
#pragma unroll 8
        for (int r = 32 * part; r < 32 * part + 32; ++r) s += dmu[r * 16 + o];
        s += __shfl_xor(s, 16, kWave);
        s += __shfl_xor(s, 32, kWave);
        if (lane < kActA) wp[kActA * kBN + lane] = s;
    }
    const int c = t & (kBN - 1), rh = t >> 8;  // dW column c over the 32 rows of buffer rh (wave-uniform)
    float wacc[kActA];
#pragma unroll
    for (int o = 0; o < kActA; ++o) wacc[o] = 0.f;
    auto dw_pass = [&](int i) {  // 3 broadcast d mu reads + 1 H read per 12 FMAs
        const float* sb = reinterpret_cast<const float*>(rh ? lds1 : lds0);
#pragma unroll 4
        for (int l = 0; l < 32; ++l) {
            const float hv = sb[act_stage_idx(l, c >> 2) + (c & 3)];
            const float4* dr = reinterpret_cast<const float4*>(dmu + (rh * 64 + i * 32 + l) * 16);
            const float4 d0 = dr[0], d1 = dr[1], d2 = dr[2];
            const float dd[kActA] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, d2.x, d2.y, d2.z, d2.w};
#pragma unroll
            for (int o = 0; o < kActA; ++o) wacc[o] = fmaf(dd[o], hv, wacc[o]);
        }
    };
    bf16x8 wa[2][3];
    auto load_wa = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int qq = 0; qq < 3; ++qq)
                wa[j][qq] = read_frag<bf16x8>(reinterpret_cast<const char*>(ap.w_t_img) + qq * kX6PlaneB,
                                              wn * 64 + j * 32 + l32, h);
    };
    auto dmu_frag = [&](int i, bf16x8 (&vb)[3]) {
        const float* r = dmu + (wm * 64 + i * 32 + l32) * 16 + 8 * h;
        const float4 v0 = *reinterpret_cast<const float4*>(r);
        const float4 v1 = *reinterpret_cast<const float4*>(r + 4);
        uint2 lo[3], hi[3];
        split4(v0, lo[0], lo[1], lo[2]);
        split4(v1, hi[0], hi[1], hi[2]);
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) vb[qq] = __builtin_bit_cast(bf16x8, make_uint4(lo[qq].x, lo[qq].y, hi[qq].x, hi[qq].y));
    };
    // dZ of block (i, j) from H values hv (C^T layout): in place over the wave's stage positions, then whole lines out
    auto dz_block = [&](int i, int j, const bf16x8 (&vb)[3], const f32x16& hv) {
        const f32x16 dacc = mfma_x6(wa[j], vb, f32x16{});
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float z = dacc[4 * g + e], hh = hv[4 * g + e];
                o[e] = hh > 0.f ? z : z * (hh + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
            }
            *reinterpret_cast<f32x4*>(stg + act_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h)) = o;
        }
        __builtin_amdgcn_wave_barrier();  // one wave's LDS accesses execute in order
        float* ct = p.c + (row0 + wm * 64 + i * 32) * kBN + (wn * 64 + j * 32);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sr = 8 * k + (lane >> 3), cq = lane & 7;
            const f32x4 v = *reinterpret_cast<const f32x4*>(stg + act_stage_idx(sr, wn * 16 + j * 8 + cq));
            f32x4* dst = reinterpret_cast<f32x4*>(ct + static_cast<uint32_t>(sr * kBN + 4 * cq));
            if (p.nt) __builtin_nontemporal_store(v, dst);
            else *dst = v;
        }
        __builtin_amdgcn_wave_barrier();
    };
    load_wa();
    dw_pass(1);
    __syncthreads();  // every wave's reads of the i = 1 stage done
    {
        bf16x8 vb[3];
        dmu_frag(1, vb);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x16 hv;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 h4 = *reinterpret_cast<const f32x4*>(stg + act_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h));
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[4 * g + e] = h4[e];
            }
            dz_block(1, j, vb, hv);
        }
    }
    stage_half(0);
    __syncthreads();  // the i = 0 stage complete
    dw_pass(0);
    __syncthreads();  // every wave's reads of the i = 0 stage done
    {
        bf16x8 vb[3];
        dmu_frag(0, vb);
#pragma unroll
        for (int j = 0; j < 2; ++j) dz_block(0, j, vb, acc[0][j]);
    }
    // ---- 4. per-tile partials: dW rows (coalesced over c), then the loss terms over the grid
    __syncthreads();  // the stages are no longer read: the buffer-1 half of dW goes through LDS
    float* dwx = reinterpret_cast<float*>(lds0);  // [12][256]
    if (rh == 1)
#pragma unroll
        for (int o = 0; o < kActA; ++o) dwx[o * kBN + c] = wacc[o];
    __syncthreads();
    if (rh == 0)
#pragma unroll
        for (int o = 0; o < kActA; ++o) wp[o * kBN + c] = wacc[o] + dwx[o * kBN + c];
    double v = 0.0;
    if (t < kActCols) {
        v = wstat[t];
#pragma unroll
        for (int w = 1; w < 8; ++w) v += wstat[w * kActCols + t];
    }
    // groups of 64 tiles up to 4096 tiles (C3's 3072), of 128 above (C4's 131,072 envs on one GPU: 6144 tiles)
    const bool folded_ok = gridDim.x > kFoldGroup * kFoldGroup
                               ? fold_grid_partials<kActCols, 2 * kFoldGroup>(ap.partials, ap.tickets,
                                                                               static_cast<int>(gridDim.x), kActCols, v,
                                                                               folded, flag)
                               : fold_grid_partials<kActCols>(ap.partials, ap.tickets, static_cast<int>(gridDim.x),
                                                              kActCols, v, folded, flag);
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
        if (t < kActA) ap.grad_sigma[t] = static_cast<float>(folded[4 + t]);
    }
}

// ---- The actor head for any action count A = p.nout in [kActMinA, kActMaxA] (12 keeps the form above) -----------------
// The same tile, phases and LDS buffers on the 16-wide padded problem.  APL = ceil(A / 4) actions per lane of a row's
// quad: lane q holds actions APL q + k (k < APL) that are < A.  A masked action loads nothing from global memory,
// computes on finite stand-ins (sigma 1, everything else 0), adds to no sum, and its d mu is an exact 0 in the
// [128][16] tile (with the columns 4 APL .. 15), never in global memory.
// LDS at A = 16: red [wm][wn][i][16][32] fills b0 [0, 32K) (the stride is kActMaxA whatever A is); wstat [8 waves][20],
// folded [20] and the flag take b0 [32768, 34212); the side area (bias, then kActSideRows rows of kActMaxA floats:
// output bias, sigma, old sigma of sample 0, the loss's per-action constants, the entropy) lives at b0 [36864, 38656)
// -- read through the whole loss, disjoint from wstat; the d mu tile is b1 [32K, 40K); dwx [A][256] is b0 [0, 16K) after the stages are dead.
// mu: linear_fwd_out_ex's bits at nout = A (the NR = 4 output layer).  d mu: kernels.ppo_loss_fwd_bwd's bits -- the
// log-prob sums per lane and then over the quad where that function takes ppo_loss_quad_kernel<APL> (A = 4 APL), and
// in action order 0 .. A - 1 (ppo_loss_kernel) everywhere else: the quad's terms arrive by DPP broadcasts.
template <int J>
__device__ __forceinline__ float quad_bcast(float v) {  // lane J of the quad, in every lane of it (quad_perm [J, J, J, J])
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), J * 0x55, 0xF, 0xF, false));
}

template <int APL, int... Is>
__device__ __forceinline__ void quad_terms(const float (&v)[APL], float (&out)[4 * APL],
                                           std::integer_sequence<int, Is...>) {
    ((out[Is] = quad_bcast<Is / APL>(v[Is % APL])), ...);
}

template <int APL, int NW>
__device__ __forceinline__ void actor_head_any_epilogue(const GemmParams& p, const ActorParams& ap,
                                                        f32x16 (&acc)[2][2], char* lds0, char* lds1, const float* xsb,
                                                        int wm, int wn, int lane, int wave, int64_t row0) {
    constexpr int QA = 4 * APL;             // d mu columns the quad's lanes write
    constexpr int kRed = kActMaxA * 32;     // floats of one (wm, wn, i) reduction tile
    constexpr int kWs = kActMaxCols;        // stride of a wave's loss partials
    constexpr int kN = 64 * NW;             // = p.N: row stride of dz and of the dW partial rows
    static_assert(NW >= 1 && NW <= 4, "actor head: N = 64, 128, 192 or 256");
    static_assert(APL >= 2 && APL <= 4 && QA <= kActMaxA, "actor head: 5 to 16 actions");
    static_assert(2 * 4 * 2 * kRed * 4 <= 32768, "actor head: red below the loss partials");
    const int A = p.nout;  // wave-uniform
    // NW < 4 (the narrow head): a wave column past N holds no H column -- its output-layer partials are exact zeros
    // (what linear_fwd_out_ex's zero-padded columns give: mu keeps its four terms in their order), it owns no dW or
    // dZ column, and it takes every barrier and its rows of the loss like any other wave
    const bool live = NW == 4 || wn < NW;  // wave-uniform
    const int cols = 4 + A;
    const int l32 = lane & 31, h = lane >> 5;
    const int t = threadIdx.x;
    float* red = reinterpret_cast<float*>(lds0);
    float* dmu = reinterpret_cast<float*>(lds1 + 32768);
    double* wstat = reinterpret_cast<double*>(lds0 + 32768);  // [8 waves][kWs]
    double* folded = wstat + 8 * kWs;                         // [kWs]
    int* flag = reinterpret_cast<int*>(folded + kWs);
    float* const stg = reinterpret_cast<float*>(wm ? lds1 : lds0);  // this wave row's half-tile H stage
    // ---- 0. the loss's per-action constants, once per tile: lane a of the last wave evaluates sigma_consts and
    // kl_fast_consts of action a (a slot past A: of sigma 1) into the side area's rows, and the entropy of a row (the
    // sum over the A actions in order) -- the values every lane of ppo_loss_quad_kernel computes for itself
    if (t >= kThreads - kWave && t < kThreads - kWave + kActMaxA) {
        float* side = const_cast<float*>(xsb) + kBN;
        const int a = t - (kThreads - kWave);
        const bool in = a < A;
        const float sv = side[kSideSigma * kActMaxA + a], o0 = side[kSideOldSigma * kActMaxA + a];
        const SigmaConsts c = sigma_consts(in ? sv : 1.0f);
        const KlFastConsts f = kl_fast_consts(c.s, in ? o0 : 1.0f, ap.kl_fast);
        side[kSideSigma * kActMaxA + a] = c.s;
        side[kSideLs * kActMaxA + a] = c.ls;
        side[kSideInvDen * kActMaxA + a] = c.inv_den;
        side[kSideInvS * kActMaxA + a] = c.inv_s;
        side[kSideInvS3 * kActMaxA + a] = c.inv_s3;
        side[kSideKlOs * kActMaxA + a] = f.os;
        side[kSideKlT1 * kActMaxA + a] = f.t1;
        side[kSideKlD * kActMaxA + a] = f.D;
        side[kSideKlRD * kActMaxA + a] = f.rD;
        float ent = 0.0f;
#pragma unroll
        for (int b = 0; b < kActMaxA; ++b) {
            const float lb = __shfl(c.ls, b, kWave);  // lanes 0..15 of this wave are all here
            if (b < A) ent = __fadd_rn(ent, entropy_term(lb));
        }
        if (a == 0) side[kSideEnt * kActMaxA] = ent;
    }
    // ---- 1. H and the output layer's partials
    const uint4* oimg = p.oimg + wn * (2 * 2 * 3 * 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
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
                for (int q = 0; q < 3; ++q) {
                    vb[q] = __builtin_bit_cast(bf16x8, make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y));
                    wa[q] = __builtin_bit_cast(bf16x8, oimg[((j * 2 + s2) * 3 + q) * 64 + lane]);
                }
                oacc = mfma_x6(wa, vb, oacc);
                __builtin_amdgcn_sched_barrier(0);  // one k step at a time: its planes die before the next split
            }
        }
        float* rd = red + ((wm * 4 + wn) * 2 + i) * kRed;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
            rd[o * 32 + l32] = oacc[r];  // o < kActMaxA: the rows from A on (zero rows of the image) are never read
        }
    }
    // ---- 2. mu and the loss of row rl on lanes q = 0..3 (actions a0 .. a0 + APL - 1 below A)
    const int rl = t >> 2, q = t & 3, a0 = APL * q;
    const int64_t row = row0 + rl;
    const float* xact = xsb + kBN;  // [obias | sigma | old_sigma of sample 0] x kActMaxA (prologue)
    bool ok[APL];
    int ak[APL];  // a masked slot works on the last action's data (finite, in bounds) and stores and adds nothing
#pragma unroll
    for (int k = 0; k < APL; ++k) {
        ok[k] = a0 + k < A;
        ak[k] = min(a0 + k, A - 1);
    }
    // the tile's rows of the [M, A] operands: wave-uniform bases and 32-bit element offsets
    const int64_t tile0 = row0 * A;
    const uint32_t e0 = static_cast<uint32_t>(rl * A);
    __syncthreads();  // red and the per-action constants complete
    float mu[APL];
#pragma unroll
    for (int k = 0; k < APL; ++k) {
        const float* b = red + ((rl >> 6) * 4 * 2 + ((rl & 63) >> 5)) * kRed + ak[k] * 32 + (rl & 31);
        const float sum = ((b[0] + b[2 * kRed]) + b[4 * kRed]) + b[6 * kRed];
        mu[k] = sum + xact[ak[k]];
        if (ok[k]) (p.y + tile0)[e0 + ak[k]] = mu[k];
    }
    float x[APL], om[APL], os[APL];
#pragma unroll
    for (int k = 0; k < APL; ++k) {
        x[k] = (ap.actions + tile0)[e0 + ak[k]];
        om[k] = (ap.old_mu + tile0)[e0 + ak[k]];
        os[k] = (ap.old_sigma + tile0)[e0 + ak[k]];
    }
    const float old_logp = ap.old_logp[row], adv = ap.adv[row], V = ap.values[row], tv = ap.target_values[row],
                R = ap.returns[row];
    __syncthreads();  // red read: buffer 0 takes the H stage
    auto stage_half = [&](int i) {
        if (!live) return;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 hv = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                *reinterpret_cast<f32x4*>(stg + act_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h)) = hv;
            }
    };
    stage_half(1);
    // the loss of the row on its quad: ppo_loss_common.h's per-sample expressions (SHARED = true) on the per-action
    // constants of the side area (read where they are used: none is held through the loss)
    auto cst = [&](int r, int a) { return xact[r * kActMaxA + a]; };
    float d[APL], term[APL], klpart = 0.0f;
    bool kl_slow = false;
#pragma unroll
    for (int k = 0; k < APL; ++k) {
        d[k] = x[k] - mu[k];
        term[k] = logp_term(d[k], cst(kSideInvDen, ak[k]), cst(kSideLs, ak[k]));
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
        for (int k = 0; k < APL; ++k) {
            const float kt = kl_term_exact(cst(kSideSigma, ak[k]), os[k], mu[k], om[k]);
            if (ok[k]) klpart = __fadd_rn(klpart, kt);
        }
    }
    const float ent_shared = cst(kSideEnt, 0);
    float logp = 0.0f;
    if (A == QA) {  // ppo_loss_quad_kernel<APL>'s order: the lane's APL terms, then the quad tree
        float lpart = 0.0f;
#pragma unroll
        for (int k = 0; k < APL; ++k) lpart += term[k];
        logp = quad_sum(lpart);
    } else {  // ppo_loss_kernel's order (tree_sum over the A terms), every lane of the quad the same sum
        float tq[QA];
        quad_terms<APL>(term, tq, std::make_integer_sequence<int, QA>{});
        logp = tree_sum<QA>(tq, A);
    }
    float gj, vterm;
    const float sterm = surrogate(logp, old_logp, adv, ap.ratio_lo, ap.ratio_hi, ap.g_surr, gj);
    // the value loss term only: its gradient is the critic head's (rslrl_value_head_fwd_bwd), so g_value is unused
    (void)value_loss(V, tv, R, ap.clipped_value, ap.clip, 0.0f, vterm);
    float gsg[APL];
#pragma unroll
    for (int k = 0; k < APL; ++k) {
        float gm, gs;
        normal_grads(d[k], cst(kSideInvDen, ak[k]), cst(kSideInvS, ak[k]), cst(kSideInvS3, ak[k]), gj, ap.g_ent, gm,
                     gs);
        gsg[k] = ok[k] ? gs : 0.0f;
        dmu[rl * 16 + a0 + k] = ok[k] ? gm : 0.0f;
        if (ap.grad_mu && ok[k]) (ap.grad_mu + tile0)[e0 + ak[k]] = gm;
    }
    if (q == 3) {
#pragma unroll
        for (int c4 = APL; c4 < 4; ++c4)
            *reinterpret_cast<float4*>(dmu + rl * 16 + 4 * c4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    {
        const double s_surr = wave_sum(static_cast<double>(q == 0 ? sterm : 0.0f));
        const double s_val = wave_sum(static_cast<double>(q == 0 ? vterm : 0.0f));
        const double s_ent = wave_sum(static_cast<double>(q == 0 ? ent_shared : 0.0f));
        const double s_kl = wave_sum(static_cast<double>(ap.compute_kl ? klpart : 0.0f));
        if (lane == 0) {
            wstat[wave * kWs + 0] = s_surr;
            wstat[wave * kWs + 1] = s_val;
            wstat[wave * kWs + 2] = s_ent;
            wstat[wave * kWs + 3] = s_kl;
        }
#pragma unroll
        for (int k = 0; k < APL; ++k) {
            double v = static_cast<double>(gsg[k]);
#pragma unroll
            for (int off = 4; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
            if (lane < 4 && APL * lane + k < A) wstat[wave * kWs + 4 + APL * lane + k] = v;
        }
    }
    __syncthreads();  // the d mu tile and the i = 1 stage complete
    // ---- 3. output-layer backward, half i = 1 (staged) then i = 0 (registers)
    float* wp = ap.wpart + static_cast<int64_t>(blockIdx.x) * act_tile_floats(A, kN);
    if (wave == 0) {  // db = column sums of d mu: lane (o, quarter) adds its 32 rows in order, then the quarters
        const int o = lane & 15, part = lane >> 4;
        float s = 0.f;
#pragma unroll 8
        for (int r = 32 * part; r < 32 * part + 32; ++r) s += dmu[r * 16 + o];
        s += __shfl_xor(s, 16, kWave);
        s += __shfl_xor(s, 32, kWave);
        if (lane < ((A + 3) & ~3)) wp[A * kN + lane] = s;  // the row's padding: sums of the tile's zero columns
    }
    const int c = t & (kBN - 1), rh = t >> 8;  // dW column c over the 32 rows of buffer rh (wave-uniform)
    float wacc[QA];
#pragma unroll
    for (int o = 0; o < QA; ++o) wacc[o] = 0.f;
    auto dw_pass = [&](int i) {  // APL broadcast d mu reads + 1 H read per QA FMAs
        const float* sb = reinterpret_cast<const float*>(rh ? lds1 : lds0);
#pragma unroll 4
        for (int l = 0; l < 32; ++l) {
            const float hv = sb[act_stage_idx(l, c >> 2) + (c & 3)];
            const float4* dr = reinterpret_cast<const float4*>(dmu + (rh * 64 + i * 32 + l) * 16);
#pragma unroll
            for (int g = 0; g < APL; ++g) {
                const float4 d4 = dr[g];
                wacc[4 * g] = fmaf(d4.x, hv, wacc[4 * g]);
                wacc[4 * g + 1] = fmaf(d4.y, hv, wacc[4 * g + 1]);
                wacc[4 * g + 2] = fmaf(d4.z, hv, wacc[4 * g + 2]);
                wacc[4 * g + 3] = fmaf(d4.w, hv, wacc[4 * g + 3]);
            }
        }
    };
    if constexpr (NW == 4) {
        bf16x8 wa[2][3];
        auto load_wa = [&]() {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int qq = 0; qq < 3; ++qq)
                    wa[j][qq] = read_frag<bf16x8>(reinterpret_cast<const char*>(ap.w_t_img) + qq * kX6PlaneB,
                                                  wn * 64 + j * 32 + l32, h);
        };
        auto dmu_frag = [&](int i, bf16x8 (&vb)[3]) {
            const float* r = dmu + (wm * 64 + i * 32 + l32) * 16 + 8 * h;
            const float4 v0 = *reinterpret_cast<const float4*>(r);
            const float4 v1 = *reinterpret_cast<const float4*>(r + 4);
            uint2 lo[3], hi[3];
            split4(v0, lo[0], lo[1], lo[2]);
            split4(v1, hi[0], hi[1], hi[2]);
#pragma unroll
            for (int qq = 0; qq < 3; ++qq) vb[qq] = __builtin_bit_cast(bf16x8, make_uint4(lo[qq].x, lo[qq].y, hi[qq].x, hi[qq].y));
        };
        // dZ of block (i, j) from H values hv (C^T layout): in place over the wave's stage positions, then whole lines out
        auto dz_block = [&](int i, int j, const bf16x8 (&vb)[3], const f32x16& hv) {
            const f32x16 dacc = mfma_x6(wa[j], vb, f32x16{});
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 o;
#pragma unroll
                for (int ee = 0; ee < 4; ++ee) {
                    const float z = dacc[4 * g + ee], hh = hv[4 * g + ee];
                    o[ee] = hh > 0.f ? z : z * (hh + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
                }
                *reinterpret_cast<f32x4*>(stg + act_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h)) = o;
            }
            __builtin_amdgcn_wave_barrier();  // one wave's LDS accesses execute in order
            float* ct = p.c + (row0 + wm * 64 + i * 32) * kBN + (wn * 64 + j * 32);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sr = 8 * k + (lane >> 3), cq = lane & 7;
                const f32x4 v = *reinterpret_cast<const f32x4*>(stg + act_stage_idx(sr, wn * 16 + j * 8 + cq));
                f32x4* dst = reinterpret_cast<f32x4*>(ct + static_cast<uint32_t>(sr * kBN + 4 * cq));
                if (p.nt) __builtin_nontemporal_store(v, dst);
                else *dst = v;
            }
            __builtin_amdgcn_wave_barrier();
        };
        load_wa();
        dw_pass(1);
        __syncthreads();  // every wave's reads of the i = 1 stage done
        {
            bf16x8 vb[3];
            dmu_frag(1, vb);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x16 hv;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 h4 = *reinterpret_cast<const f32x4*>(stg + act_stage_idx(l32, wn * 16 + j * 8 + 2 * g + h));
#pragma unroll
                    for (int ee = 0; ee < 4; ++ee) hv[4 * g + ee] = h4[ee];
                }
                dz_block(1, j, vb, hv);
            }
        }
        stage_half(0);
        __syncthreads();  // the i = 0 stage complete
        dw_pass(0);
        __syncthreads();  // every wave's reads of the i = 0 stage done
        {
            bf16x8 vb[3];
            dmu_frag(0, vb);
#pragma unroll
            for (int j = 0; j < 2; ++j) dz_block(0, j, vb, acc[0][j]);
        }
    } else {
        // The narrow head: dZ on the VALU inside the dW pass, in place over H in the stage.  Thread (c, rh) holds
        // W_out[o][c] and forms z = sum over o of d mu[l][o] W_out[o][c] as the separate output-layer backward does
        // (out_bwd_valu_body: one fp32 FMA chain from 0 in action order over A rounded up to 4; the tile's d mu columns
        // from A on are zeros) and dZ = z ELU'(H): that launch's bits, so everything behind the last hidden layer
        // is the same with and without the head (the x6 products of the 256-wide form round differently).  Each wave
        // reads and writes only its own 32 x 64 region of the stage.
        float wcol[QA];  // W_out[o][c] = the sum of the image's three planes (exact: they were split from it)
#pragma unroll
        for (int o = 0; o < QA; ++o) wcol[o] = 0.f;
        if (live) {
#pragma unroll
            for (int lh = 0; lh < (QA + 7) / 8; ++lh) {
                uint4 q3[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) q3[pl] = ap.w_t_img[(pl * kX6PlaneB + swz(c, lh)) / 16];
                const uint32_t* u0 = reinterpret_cast<const uint32_t*>(&q3[0]);
                const uint32_t* u1 = reinterpret_cast<const uint32_t*>(&q3[1]);
                const uint32_t* u2 = reinterpret_cast<const uint32_t*>(&q3[2]);
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    if (8 * lh + jj >= QA) break;
                    auto pick = [jj](const uint32_t* u) {
                        const uint32_t x = u[jj >> 1];
                        return __uint_as_float((jj & 1) ? (x & 0xffff0000u) : (x << 16));
                    };
                    wcol[8 * lh + jj] = (pick(u0) + pick(u1)) + pick(u2);
                }
            }
        }
        auto dwz_pass = [&](int i) {
            if (!live) return;  // column c belongs to wave column wn
            float* sb = reinterpret_cast<float*>(rh ? lds1 : lds0);
#pragma unroll 4
            for (int l = 0; l < 32; ++l) {
                float* hp = sb + act_stage_idx(l, c >> 2) + (c & 3);
                const float hv = *hp;
                const float4* dr = reinterpret_cast<const float4*>(dmu + (rh * 64 + i * 32 + l) * 16);
                float z = 0.f;
#pragma unroll
                for (int g = 0; g < APL; ++g) {
                    const float4 d4 = dr[g];
                    wacc[4 * g] = fmaf(d4.x, hv, wacc[4 * g]);
                    wacc[4 * g + 1] = fmaf(d4.y, hv, wacc[4 * g + 1]);
                    wacc[4 * g + 2] = fmaf(d4.z, hv, wacc[4 * g + 2]);
                    wacc[4 * g + 3] = fmaf(d4.w, hv, wacc[4 * g + 3]);
                    z = fmaf(d4.x, wcol[4 * g], z);
                    z = fmaf(d4.y, wcol[4 * g + 1], z);
                    z = fmaf(d4.z, wcol[4 * g + 2], z);
                    z = fmaf(d4.w, wcol[4 * g + 3], z);
                }
                *hp = hv > 0.f ? z : z * (hv + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
            }
        };
        auto store_half = [&](int i) {  // the wave's 32 x 64 dZ out of the stage as whole lines, at row stride N
            if (!live) return;
            __builtin_amdgcn_wave_barrier();  // one wave's LDS accesses execute in order
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float* ct = p.c + (row0 + wm * 64 + i * 32) * kN + (wn * 64 + j * 32);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sr = 8 * k + (lane >> 3), cq = lane & 7;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(stg + act_stage_idx(sr, wn * 16 + j * 8 + cq));
                    f32x4* dst = reinterpret_cast<f32x4*>(ct + static_cast<uint32_t>(sr * kN + 4 * cq));
                    if (p.nt) __builtin_nontemporal_store(v, dst);
                    else *dst = v;
                }
            }
            __builtin_amdgcn_wave_barrier();
        };
        dwz_pass(1);
        __syncthreads();  // (the regions are per wave; the barriers stand where the 256-wide form has them)
        store_half(1);
        stage_half(0);
        __syncthreads();
        dwz_pass(0);
        __syncthreads();
        store_half(0);
    }
    // ---- 4. per-tile partials: dW rows (coalesced over c), then the loss terms over the grid
    __syncthreads();  // the stages are no longer read: the buffer-1 half of dW goes through LDS
    float* dwx = reinterpret_cast<float*>(lds0);  // [A][256]
    if (rh == 1 && live)
#pragma unroll
        for (int o = 0; o < QA; ++o)
            if (o < A) dwx[o * kBN + c] = wacc[o];
    __syncthreads();
    if (rh == 0 && live)
#pragma unroll
        for (int o = 0; o < QA; ++o)
            if (o < A) wp[o * kN + c] = wacc[o] + dwx[o * kBN + c];
    double v = 0.0;
    if (t < cols) {
        v = wstat[t];
#pragma unroll
        for (int w = 1; w < 8; ++w) v += wstat[w * kWs + t];
    }
    // groups of 64 tiles up to 4096 tiles, of 128 above
    const bool folded_ok = gridDim.x > kFoldGroup * kFoldGroup
                               ? fold_grid_partials<kActMaxCols, 2 * kFoldGroup>(ap.partials, ap.tickets,
                                                                                  static_cast<int>(gridDim.x), cols, v,
                                                                                  folded, flag)
                               : fold_grid_partials<kActMaxCols>(ap.partials, ap.tickets, static_cast<int>(gridDim.x),
                                                                 cols, v, folded, flag);
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
}

// The critic's last hidden layer + value head + d(value loss)/dV + the value head's backward (dZ of the last hidden
// layer and the head's weight-gradient partials) in one launch (rslrl_value_head_fwd_bwd): full 128-row tiles, x6.
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_value_head_kernel(GemmParams p, const uint4* __restrict__ bimg) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    mlp_gemm_x6_body<kEpiBiasEluOut, true, 1, 3, true, 0, 1>(p, bimg, lds_b0, lds_b1);
}

// The actor's last hidden layer + output layer + the PPO loss + the output layer's backward in one launch
// (rslrl_actor_head_fwd_bwd; actor_head_epilogue): full 128-row tiles, x6.
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_actor_head_kernel(GemmParams p, const uint4* __restrict__ bimg,
                                                                           ActorParams ap) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    mlp_gemm_x6_body<kEpiBiasEluOut, true, 4, 3, true, 0, 2>(p, bimg, lds_b0, lds_b1, &ap);
}

// The same launch for p.nout = 5 .. 16 actions but 12, APL = ceil(p.nout / 4) per quad lane (actor_head_any_epilogue)
template <int APL>
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_actor_head_any_kernel(GemmParams p,
                                                                               const uint4* __restrict__ bimg,
                                                                               ActorParams ap) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    mlp_gemm_x6_body<kEpiBiasEluOut, true, 4, 3, true, 0, kHeadActorAny + APL>(p, bimg, lds_b0, lds_b1, &ap);
}

// The narrow heads (rslrl_value_head_fwd_bwd_n, rslrl_actor_head_fwd_bwd_n): a last hidden layer of N = 64 NW < 256
// columns on the same 128 x 256 tile over the zero-padded images RSLRL_LINEAR_FWD_OUT already runs.  NW of the four
// wave columns are live; the others skip the main loop's MFMAs, the ELU/split epilogue and the dW/dZ work (wave-uniform
// branches), reach every barrier and take their rows of the loss.  dz [M, N] and the dW partial rows are written at
// stride N.  Every action count takes the any-A epilogue (12 included: the same mu, d mu and partials as the 12-action
// form).  The actor's dZ is formed on the VALU inside the dW pass with the separate output-layer backward's fp32 FMA
// chain -- that launch's bits, where the 256-wide form's x6 MFMA rounds differently -- so the gradients behind the last
// hidden layer do not depend on whether the head ran.
template <int NW>
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_value_head_n_kernel(GemmParams p,
                                                                             const uint4* __restrict__ bimg) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    mlp_gemm_x6_body<kEpiBiasEluOut, true, 1, 3, true, 0, 1, NW>(p, bimg, lds_b0, lds_b1);
}

template <int APL, int NW>
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_actor_head_n_kernel(GemmParams p,
                                                                             const uint4* __restrict__ bimg,
                                                                             ActorParams ap) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, 3>()];
    mlp_gemm_x6_body<kEpiBiasEluOut, true, 4, 3, true, 0, kHeadActorAny + APL, NW>(p, bimg, lds_b0, lds_b1, &ap);
}

// The actor's and the critic's fused last hidden + output layer in one launch (blockIdx.y): the two output widths
// take different epilogues (NR 4: MFMA output layer, e.g. 12 actions; NR 1: VALU, <= 4 outputs, e.g. the value
// head), one body each over the shared LDS buffers.  At the rollout's 16,384 rows per GPU each alone fills a
// quarter of the workgroup slots.
template <bool FULL, int MINW, int NR0, int NR1, int PL>
__global__ __launch_bounds__(kThreads, MINW) void mlp_gemm_x6_out_pair_kernel(GemmPair b) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<kEpiBiasEluOut, PL>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<kEpiBiasEluOut, PL>()];
    // (distinct opaque markers open the two branches: otherwise the bodies' common index arithmetic is hoisted
    // above the branch, lives through either body and spills)
    if (blockIdx.y == 0) {
        asm volatile("; out pair: problem 0" ::: "memory");
        mlp_gemm_x6_body<kEpiBiasEluOut, FULL, NR0, PL>(b.p[0], b.img[0], lds_b0, lds_b1);
    } else {
        asm volatile("; out pair: problem 1" ::: "memory");
        mlp_gemm_x6_body<kEpiBiasEluOut, FULL, NR1, PL>(b.p[1], b.img[1], lds_b0, lds_b1);
    }
}

int out_fwd_occupancy() {  // tuning knob: RSLRL_OUT_FWD_OCC=2|4 (default 4)
    static const int v = [] {
        const char* e = std::getenv("RSLRL_OUT_FWD_OCC");
        return (e && std::atoi(e) == 2) ? 2 : 4;
    }();
    return v;
}

template <int PL>
int launch_fwd_out(const GemmParams& p, const void* bimage, hipStream_t st) {
    constexpr int EPI = kEpiBiasEluOut;
    const int64_t tiles = ceil_div(p.M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    const dim3 g(static_cast<unsigned>(tiles)), b(kThreads);
    const uint4* img = static_cast<const uint4*>(bimage);
    const bool fullm = p.M % kBM == 0 && p.K % kKC == 0;
    auto go = [&](auto nr) {  // NR 1: VALU output layer (nout <= 4), 4: MFMA output layer
        constexpr int NR = decltype(nr)::value;
        if (out_fwd_occupancy() == 2) {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, true, 2, NR, PL>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, false, 2, NR, PL>), g, b, 0, st, p, img);
        } else {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, true, 4, NR, PL>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, false, 4, NR, PL>), g, b, 0, st, p, img);
        }
    };
    if (p.nout <= 4) go(std::integral_constant<int, 1>{});
    else go(std::integral_constant<int, 4>{});
    return launch_status();
}

// (MINW 2: both epilogues in one kernel do not fit 128 registers without spills; the pair is only taken when its
// tiles are at most one per CU, where the occupancy limit costs nothing)
template <bool FULL, int NR0>
void launch_out_pair(const GemmPair& b, int nr1, dim3 g, hipStream_t st) {
    if (nr1 == 1) hipLaunchKernelGGL((mlp_gemm_x6_out_pair_kernel<FULL, 2, NR0, 1, 3>), g, dim3(kThreads), 0, st, b);
    else hipLaunchKernelGGL((mlp_gemm_x6_out_pair_kernel<FULL, 2, NR0, 4, 3>), g, dim3(kThreads), 0, st, b);
}

}  // namespace

int fwd_out_launch(const GemmParams& p, const void* bimage, int pl, hipStream_t st) {
    return pl == 2 ? launch_fwd_out<2>(p, bimage, st) : launch_fwd_out<3>(p, bimage, st);
}

void fwd_out_pair_launch(const GemmPair& b, bool fullm, dim3 g, hipStream_t st) {
    const int nr0 = b.p[0].nout <= 4 ? 1 : 4, nr1 = b.p[1].nout <= 4 ? 1 : 4;
    if (fullm) {
        if (nr0 == 1) launch_out_pair<true, 1>(b, nr1, g, st);
        else launch_out_pair<true, 4>(b, nr1, g, st);
    } else {
        if (nr0 == 1) launch_out_pair<false, 1>(b, nr1, g, st);
        else launch_out_pair<false, 4>(b, nr1, g, st);
    }
}

}  // namespace rslrl

using namespace rslrl;

extern "C" size_t rslrl_actor_head_workspace_bytes(int64_t M);

namespace {

// What the two value-head entries share behind their shape checks: the head's pointers and the loss constants into p
int value_head_params(const rslrl_linear_args_t* a, const rslrl_value_head_args_t* v, GemmParams& p) {
    if (!a->c || !v->target_values || !v->returns || !v->out_weight || !v->wgrad_partials)
        return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(v->out_weight)) return RSLRL_E_MISALIGNED;
    p.vh_tv = v->target_values;
    p.vh_ret = v->returns;
    p.vh_w = v->out_weight;
    p.vh_clip = v->clip_param;
    p.vh_g = loss_scalars(v->clip_param, v->value_loss_coef, 0.0f, a->M).g_value;
    p.vh_clipped = v->use_clipped_value_loss ? 1 : 0;
    p.wpart = v->wgrad_partials;
    p.colsum = v->colsum_partials;
    return RSLRL_OK;
}

// ... and the two actor-head entries: pointers, alignment, the workspace and the loss constants into ap
int actor_head_params(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h, void* workspace,
                      size_t workspace_bytes, ActorParams& ap) {
    if (!a->c || !h->actions || !h->old_log_prob || !h->advantages || !h->values || !h->target_values ||
        !h->returns || !h->old_mu || !h->old_sigma || !h->sigma || !h->out_weight_t_image || !h->wgrad_partials ||
        !h->grad_sigma || !h->stats || !workspace)
        return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(a->c) || !aligned16(h->out_weight_t_image) || !aligned16(workspace)) return RSLRL_E_MISALIGNED;
    if (workspace_bytes < rslrl_actor_head_workspace_bytes(a->M)) return RSLRL_E_WORKSPACE_TOO_SMALL;
    ap.actions = h->actions;
    ap.old_mu = h->old_mu;
    ap.old_sigma = h->old_sigma;
    ap.sigma = h->sigma;
    ap.old_logp = h->old_log_prob;
    ap.adv = h->advantages;
    ap.values = h->values;
    ap.target_values = h->target_values;
    ap.returns = h->returns;
    ap.w_t_img = static_cast<const uint4*>(h->out_weight_t_image);
    ap.wpart = h->wgrad_partials;
    ap.grad_sigma = h->grad_sigma;
    ap.stats = h->stats;
    ap.grad_mu = h->grad_mu;
    ap.tickets = static_cast<unsigned*>(workspace);
    ap.partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + 1024);
    const LossScalars k = loss_scalars(h->clip_param, h->value_loss_coef, h->entropy_coef, a->M);
    ap.clip = h->clip_param;
    ap.ratio_lo = k.ratio_lo;
    ap.ratio_hi = k.ratio_hi;
    ap.g_surr = k.g_surr;
    ap.g_ent = k.g_ent;
    ap.value_loss_coef = h->value_loss_coef;
    ap.entropy_coef = h->entropy_coef;
    ap.clipped_value = h->use_clipped_value_loss ? 1 : 0;
    ap.compute_kl = h->compute_kl ? 1 : 0;
    ap.kl_fast = kl_fast_enabled() ? 1 : 0;
    return RSLRL_OK;
}

// wave columns of a narrow head's N (64, 128, 192), else 0
int narrow_wave_cols(int64_t N) { return N == 64 || N == 128 || N == 192 ? static_cast<int>(N / 64) : 0; }

}  // namespace

// The critic's last hidden layer, value head, value-loss gradient and value-head backward in one launch
// (include/rslrl_amd.h).  Unsupported shapes return RSLRL_E_UNSUPPORTED before anything is launched (the caller
// then runs the separate launches).
extern "C" int rslrl_value_head_fwd_bwd(const rslrl_linear_args_t* a, const rslrl_value_head_args_t* v,
                                        rslrl_stream_t stream) {
    if (!a || !v || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    if (a->arith != RSLRL_ARITH_X6 || a->nout != 1 || a->N != kBN || a->K != 16 * kKC || a->M % kBM != 0 || !p.deep)
        return RSLRL_E_UNSUPPORTED;
    const int prc = value_head_params(a, v, p);
    if (prc) return prc;
    if (a->M == 0) return RSLRL_OK;
    const int64_t tiles = ceil_div(a->M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    if (value_head_stream_enabled() && !v->colsum_partials) {  // opt-in: the streaming main loop (mlp_fwd_stream.hip)
        const ValueHeadStreamArgs s{p.a, a->bimage, p.bias, v->out_weight, p.obias, v->target_values, v->returns,
                                    a->c, p.y, v->wgrad_partials, p.vh_clip, p.vh_g, p.vh_clipped, a->M};
        return value_head_stream(s, reinterpret_cast<hipStream_t>(stream));
    }
    hipLaunchKernelGGL(mlp_gemm_x6_value_head_kernel, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), p, static_cast<const uint4*>(a->bimage));
    return launch_status();
}

extern "C" int64_t rslrl_value_head_partial_rows(int64_t M, int32_t with_colsum) {
    if (M <= 0) return 0;
    // the same dispatch as rslrl_value_head_fwd_bwd: the streaming form never takes colsum_partials
    return value_head_stream_enabled() && !with_colsum ? value_head_stream_rows(M) : ceil_div(M, kBM);
}

// The actor's last hidden layer, output layer, the PPO loss and the output layer's backward in one launch
// (include/rslrl_amd.h).  Unsupported shapes return RSLRL_E_UNSUPPORTED before anything is launched.
extern "C" size_t rslrl_actor_head_workspace_bytes(int64_t M) {
    const int64_t tiles = ceil_div(M > 0 ? M : 0, kBM);
    const int64_t groups = ceil_div(tiles, kFoldGroup);  // >= the groups of 128 a larger grid folds in
    return 1024 + sizeof(double) * static_cast<size_t>(kActMaxCols * (tiles + groups));  // sized for 16 actions
}

extern "C" int rslrl_actor_head_fwd_bwd(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h,
                                        void* workspace, size_t workspace_bytes, rslrl_stream_t stream) {
    if (!a || !h || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    const int64_t tiles = ceil_div(a->M, kBM);
    const int A = a->nout;
    if (a->arith != RSLRL_ARITH_X6 || A < kActMinA || A > kActMaxA || h->num_actions != A || a->N != kBN ||
        a->K != 16 * kKC || a->M % kBM != 0 || a->M < 1 || !p.deep || tiles > int64_t{2 * kFoldGroup} * kFoldGroup)
        return RSLRL_E_UNSUPPORTED;
    ActorParams ap{};
    const int prc = actor_head_params(a, h, workspace, workspace_bytes, ap);
    if (prc) return prc;
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    const dim3 g(static_cast<unsigned>(tiles)), b(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint4* img = static_cast<const uint4*>(a->bimage);
    if (A == kActA) hipLaunchKernelGGL(mlp_gemm_x6_actor_head_kernel, g, b, 0, st, p, img, ap);
    else if (A <= 8) hipLaunchKernelGGL(mlp_gemm_x6_actor_head_any_kernel<2>, g, b, 0, st, p, img, ap);
    else if (A <= 12) hipLaunchKernelGGL(mlp_gemm_x6_actor_head_any_kernel<3>, g, b, 0, st, p, img, ap);
    else hipLaunchKernelGGL(mlp_gemm_x6_actor_head_any_kernel<4>, g, b, 0, st, p, img, ap);
    return launch_status();
}

// The two heads for a last hidden layer of N = 64, 128 or 192 columns (include/rslrl_amd.h): the same argument structs,
// the tiled kernels only (never the streaming forms).  Every other shape -- N = 256 included: the entries above --
// returns RSLRL_E_UNSUPPORTED before anything is launched.
extern "C" int rslrl_value_head_fwd_bwd_n(const rslrl_linear_args_t* a, const rslrl_value_head_args_t* v,
                                          rslrl_stream_t stream) {
    if (!a || !v || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    const int nw = narrow_wave_cols(a->N);
    if (a->arith != RSLRL_ARITH_X6 || !nw || a->K != 16 * kKC) return RSLRL_E_UNSUPPORTED;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    if (a->nout != 1 || a->M % kBM != 0 || !p.deep) return RSLRL_E_UNSUPPORTED;
    const int prc = value_head_params(a, v, p);
    if (prc) return prc;
    if (a->M == 0) return RSLRL_OK;
    const int64_t tiles = ceil_div(a->M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    const dim3 g(static_cast<unsigned>(tiles)), b(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint4* img = static_cast<const uint4*>(a->bimage);
    if (nw == 1) hipLaunchKernelGGL(mlp_gemm_x6_value_head_n_kernel<1>, g, b, 0, st, p, img);
    else if (nw == 2) hipLaunchKernelGGL(mlp_gemm_x6_value_head_n_kernel<2>, g, b, 0, st, p, img);
    else hipLaunchKernelGGL(mlp_gemm_x6_value_head_n_kernel<3>, g, b, 0, st, p, img);
    return launch_status();
}

namespace {
template <int NW>
void launch_actor_head_n(int A, dim3 g, hipStream_t st, const GemmParams& p, const uint4* img, const ActorParams& ap) {
    const dim3 b(kThreads);
    if (A <= 8) hipLaunchKernelGGL((mlp_gemm_x6_actor_head_n_kernel<2, NW>), g, b, 0, st, p, img, ap);
    else if (A <= 12) hipLaunchKernelGGL((mlp_gemm_x6_actor_head_n_kernel<3, NW>), g, b, 0, st, p, img, ap);
    else hipLaunchKernelGGL((mlp_gemm_x6_actor_head_n_kernel<4, NW>), g, b, 0, st, p, img, ap);
}
}  // namespace

extern "C" int rslrl_actor_head_fwd_bwd_n(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h,
                                          void* workspace, size_t workspace_bytes, rslrl_stream_t stream) {
    if (!a || !h || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    const int nw = narrow_wave_cols(a->N);
    if (a->arith != RSLRL_ARITH_X6 || !nw || a->K != 16 * kKC) return RSLRL_E_UNSUPPORTED;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    const int64_t tiles = ceil_div(a->M, kBM);
    const int A = a->nout;
    if (A < kActMinA || A > kActMaxA || h->num_actions != A || a->M % kBM != 0 || a->M < 1 || !p.deep ||
        tiles > int64_t{2 * kFoldGroup} * kFoldGroup)
        return RSLRL_E_UNSUPPORTED;
    ActorParams ap{};
    const int prc = actor_head_params(a, h, workspace, workspace_bytes, ap);
    if (prc) return prc;
    const dim3 g(static_cast<unsigned>(tiles));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint4* img = static_cast<const uint4*>(a->bimage);
    if (nw == 1) launch_actor_head_n<1>(A, g, st, p, img, ap);
    else if (nw == 2) launch_actor_head_n<2>(A, g, st, p, img, ap);
    else launch_actor_head_n<3>(A, g, st, p, img, ap);
    return launch_status();
}
