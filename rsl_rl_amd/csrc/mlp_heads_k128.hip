// The PPO update's fused heads for a last hidden layer with 128 inputs (Linear(128, N) + ELU + the output Linear of
// rsl_rl/networks/mlp.py:106-114; N = 64 or 128: the tails of [128, 128, 128], [256, 128, 128] and [256, 128, 64]), one
// launch per network for the last hidden layer, the output layer, the loss term and the output layer's backward:
//   rslrl_value_head_fwd_bwd_k128   critic: V, d(value loss)/dV, dZ of the last hidden layer, the [dW | db] partials
//   rslrl_actor_head_fwd_bwd_k128   actor: mu, the PPO loss and its statistics, d mu, d sigma, dZ, the [dW | db] partials
// The 256-deep heads (mlp_heads.hip) are a 128 x 256 tile of 8 waves around a 16-chunk look-ahead loop that stages both
// operands through LDS.  At K = 128 a tile's whole x fits LDS as three bf16 planes and the weights are 8 chunks that stay
// in L2, so the shape gets the geometry of the 128-wide hidden backward (mlp_bwd_fused_n.hip) instead:
//
// Workgroup = 4 waves (one per SIMD), a 64-row tile, 62.3 KiB of LDS, at most 256 registers per lane -> two workgroups
// per CU whose waves are never at the same barrier: one workgroup's loss and VALU backward run beside the other's
// MFMAs.  A workgroup walks a slice of consecutive tiles (kh_tiles_per) and keeps across it, in registers, what the
// tiled heads write per tile: the output layer's dW accumulators, db, the loss statistics and d sigma.  One partial
// row and one column of loss partials per slice.
//
// Wave w = (ib, wn) = (w >> 1, w & 1) owns rows [32 ib, 32 ib + 32) and the H columns [64 wn, 64 wn + 64) of the tile:
// the 64-column group whose output-layer partial linear_fwd_out_ex keeps in one accumulator (at N = 64 the wn = 1 waves
// hold no column: they skip the MFMAs and take their share of everything else).  Per tile:
//  1. main loop: 8 k-chunks in ascending order, Arith<3>::mfma per chunk with the weight fragment as the A operand
//     (C^T tiles, as the forward's): x fragments by ds_read_b128 from the resident planes, weight fragments (rows
//     64 wn + 32 j + l of the layout-0 image) from global memory one chunk ahead; no LDS write, no barrier.
//  2. H = ELU(acc + b) in registers; the output layer on it (actor: the NR = 4 x6 MFMA epilogue of the forward; critic:
//     its fp32 FMA chain) -> per-(ib, wn) partial tiles; H into the stage, which takes over the x planes' LDS.
//  3. thread t owns row t >> 2 (critic: t) of the tile: mu / V = ((p0 + p1) + 0) + 0 + bias -- linear_fwd_out_ex's
//     four-term sum, whose terms past N are exact zeros -- and the loss of the row on its quad of lanes
//     (ppo_loss_common.h's expressions, as actor_head_any_epilogue calls them) -> the d mu tile [64][16] / dV [64].
//  4. thread (c, rg) walks column c of its 16 N / 64 staged rows with the d mu row broadcast from LDS:
//     dW[o][c] += d mu[r][o] H[r][c] and z = one fp32 FMA chain from 0 in action order over A rounded up to 4,
//     dZ = z ELU'(H) in place over H (out_bwd_valu_body's expression: RSLRL_LINEAR_DGRAD_ELU_WGRAD's bits); each wave
//     then stores its region as 256-byte row segments.
//  5. the next tile's x (loaded behind phase 2, into the registers H has left) is split into the planes.
// LDS: [0, 48K) the x planes, after the main loop the H stage [64][N] fp32 and at the slice's end the dW row groups;
// [48K, 62.3K) the side area: hidden bias, per-action rows (or the value weights), the partial tiles, the d mu tile /
// dV, the loss partials of the four waves.
// x plane: [8 chunks of 16 columns][64 row slots][32 bytes], mlp_bwd_fused_n.hip's image (row m of chunk c in slot
// m ^ f(c), halves swapped on (m >> 3) & 1): the staging stores and the row-fragment reads are its, conflict free.
// H stage: row r is N floats, its float4 quads XOR-swizzled inside their group of 16 by r & 15: the C^T quad stores (16
// lanes = 16 rows of one quad), the column walk (64 lanes = 64 consecutive columns of one row) and the row-segment
// reads (16 lanes = one row's 16 quads) each cover all 64 banks once.
#include "actor_head_host.h"
#include "common.h"
#include "heads_k128_tile.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

// side area (floats from kKhXBytes): hidden bias, then the head's own
constexpr int kKhSideRows = 128;              // actor: kActSideRows rows of kActMaxA; critic: the value weights [N]
constexpr int kKhRed = kKhSideRows + 256;     // actor: [ib][wn][16][32] partial tiles; critic: [ib][wn][32]
constexpr int kKhDmu = kKhRed + 2 * 2 * kActMaxA * 32;  // actor: d mu [64][16]; critic: dV [64]
constexpr int kKhStat = kKhDmu + kKhT * kActMaxA;       // fp64: wstat [4 waves][kActMaxCols], folded [kActMaxCols], flag
constexpr int kKhSideBytes = 4 * kKhStat + 8 * (5 * kActMaxCols) + 16;
constexpr int kKhLds = kKhXBytes + kKhSideBytes;
static_assert(kActSideRows * kActMaxA <= 256, "k128 heads: the per-action rows");
static_assert(kKhLds <= 80 * 1024, "k128 heads: two workgroups per CU");
static_assert((4 * kKhStat) % 8 == 0, "k128 heads: fp64 loss partials");

// ---- the critic -------------------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(kKhThreads, 2) void value_head_k128_kernel(KhArgs a) {
    using T = KhTile<NW>;
    constexpr int kN = T::kN;
    __shared__ __attribute__((aligned(16))) char lds[kKhLds];
    const GemmParams& p = a.p;
    float* const stg = reinterpret_cast<float*>(lds);
    float* const side = reinterpret_cast<float*>(lds + kKhXBytes);
    float* const wvl = side + kKhSideRows;  // [N] the value weights, column order
    float* const red = side + kKhRed;       // [ib][wn][32] V partials
    float* const dvl = side + kKhDmu;       // [64] dV of the tile
    T tl;
    tl.init(lds, a.img);
    const int t = threadIdx.x;
    const int t_begin = blockIdx.x * a.tiles_per;
    const int t_end = min(a.tiles, t_begin + a.tiles_per);

    if (t < kN / 4) {
        reinterpret_cast<float4*>(side)[t] = *reinterpret_cast<const float4*>(p.bias + 4 * t);
        reinterpret_cast<float4*>(wvl)[t] = *reinterpret_cast<const float4*>(p.vh_w + 4 * t);
    }
    {
        float4 v[8];
        kh_load_x(p.a, static_cast<int64_t>(t_begin) * kKhT, v);
        kh_store_x(v, lds);
    }
    __syncthreads();
    const float wc = wvl[tl.c];  // this thread's column of the value weights
    const float ob = p.obias[0];
    float wsum = 0.f, dbsum = 0.f;

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t row0 = static_cast<int64_t>(tile) * kKhT;
        const bool has_next = tile + 1 < t_end;
        f32x16 acc[2];
        tl.main_loop(acc);
        float tv = 0.f, ret = 0.f;
        if (t < kKhT) {
            tv = p.vh_tv[row0 + t];
            ret = p.vh_ret[row0 + t];
        }
        kh_barrier();  // every wave has read the x planes: the stage takes them over
        if (tl.live) {
            tl.elu_bias(acc, side);
            // the value head of the forward's NR = 1 epilogue: one fp32 FMA chain over the lane's 32 columns in its
            // order (j, k step s2, element), then the two lane halves
            float oval = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int col = tl.wn * 64 + j * 32 + 4 * tl.h + 8 * (2 * s2 + (e >> 2)) + (e & 3);
                        oval = fmaf(acc[j][8 * s2 + e], wvl[col], oval);
                    }
            const float tsum = oval + __shfl_xor(oval, 32, 64);
            if (tl.h == 0) red[(tl.ib * 2 + tl.wn) * 32 + tl.l32] = tsum;
            tl.stage_h(acc, stg);
        }
        // the next tile's x into the registers H has just left: it lands behind the loss and the column walk
        float4 vn[8];
        if (has_next) kh_load_x(p.a, row0 + kKhT, vn);
        kh_barrier();  // the partials and the stage complete
        if (t < kKhT) {
            const float* b = red + (t >> 5) * 64 + (t & 31);
            // linear_fwd_out_ex's ((p0 + p1) + p2) + p3: the partials of the wave columns past N are exact zeros
            const float p1 = NW == 2 ? b[32] : 0.f;
            const float sum = ((b[0] + p1) + 0.f) + 0.f;
            const float V = sum + ob;
            p.y[row0 + t] = V;
            dvl[t] = value_loss_grad(V, tv, ret, p.vh_clipped, p.vh_clip, p.vh_g);
        }
        kh_barrier();  // dV complete
        if (tl.wave == 0) {  // db: the tile's dV in a fixed butterfly order
            float sv = dvl[tl.lane];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) sv += __shfl_xor(sv, off, 64);
            dbsum += sv;
        }
#pragma unroll 4
        for (int l = 0; l < T::kRPG; ++l) {
            const int r = T::kRPG * tl.rg + l;
            float* hp = stg + kh_stage_idx<kN>(r, tl.c >> 2) + (tl.c & 3);
            const float hh = *hp;
            const float dv = dvl[r];
            const float z = __fmaf_rn(dv, wc, 0.f);  // out_bwd_valu_body's fma chain of one term
            *hp = hh > 0.f ? z : z * (hh + 1.f);     // ELU'(x) = 1 if h > 0 else h + 1
            wsum = fmaf(dv, hh, wsum);
        }
        tl.store_dz(stg, p.c, row0, p.nt);
        __syncthreads();  // the stage is read: the next tile's planes (or the dW row groups) take the LDS
        if (has_next) {
            kh_store_x(vn, lds);
            __syncthreads();
        }
    }
    // ---- the slice's partial row [dW (N) | db | 0 0 0]: the row groups in order
    stg[tl.rg * kN + tl.c] = wsum;
    __syncthreads();
    float* wp = p.wpart + static_cast<int64_t>(blockIdx.x) * (kN + 4);
    if (t < kN) {
        float v = stg[t];
#pragma unroll
        for (int g = 1; g < T::kRG; ++g) v += stg[g * kN + t];
        wp[t] = v;
    }
    if (t < 4) wp[kN + t] = t == 0 ? dbsum : 0.f;
}

// ---- the actor: A = p.nout in [kActMinA, kActMaxA], APL = ceil(A / 4) actions per lane of a row's quad ------------------
template <int APL, int NW>
__global__ __launch_bounds__(kKhThreads, 2) void actor_head_k128_kernel(KhArgs a, ActorParams ap) {
    using T = KhTile<NW>;
    constexpr int kN = T::kN;
    constexpr int QA = 4 * APL;
    constexpr int kRed = kActMaxA * 32;  // floats of one (ib, wn) partial tile
    constexpr int kWs = kActMaxCols;
    static_assert(APL >= 2 && APL <= 4, "k128 actor head: 5 to 16 actions");
    __shared__ __attribute__((aligned(16))) char lds[kKhLds];
    const GemmParams& p = a.p;
    float* const stg = reinterpret_cast<float*>(lds);
    float* const side = reinterpret_cast<float*>(lds + kKhXBytes);
    float* const xact = side + kKhSideRows;  // kActSideRows rows of kActMaxA floats
    float* const red = side + kKhRed;        // [ib][wn][16][32]
    float* const dmu = side + kKhDmu;        // [64][16]
    double* const wstat = reinterpret_cast<double*>(side + kKhStat);  // [4 waves][kWs]
    double* const folded = wstat + 4 * kWs;
    int* const flag = reinterpret_cast<int*>(folded + kWs);
    T tl;
    tl.init(lds, a.img);
    const int t = threadIdx.x, lane = tl.lane;
    const int A = p.nout;  // wave-uniform
    const int cols = 4 + A;
    const int t_begin = blockIdx.x * a.tiles_per;
    const int t_end = min(a.tiles, t_begin + a.tiles_per);

    // ---- once per slice: the waves' loss sums (wstat: each wave adds its tiles' fp64 sums to its own row, in LDS -- 16
    // registers less through the slice than holding them), the bias, the per-action rows (lane a of the last wave: sigma_consts and kl_fast_consts of
    // action a, of sigma 1 past A, and the entropy of a row -- actor_head_any_epilogue's phase 0), the first x tile
    if (t < 4 * kWs) wstat[t] = 0.0;
    if (t < kN / 4) reinterpret_cast<float4*>(side)[t] = *reinterpret_cast<const float4*>(p.bias + 4 * t);
    if (t >= kKhThreads - kWave && t < kKhThreads - kWave + kActMaxA) {
        const int aa = t - (kKhThreads - kWave);
        const bool in = aa < A;
        const SigmaConsts c = sigma_consts(in ? ap.sigma[aa] : 1.0f);
        const KlFastConsts f = kl_fast_consts(c.s, in ? ap.old_sigma[aa] : 1.0f, ap.kl_fast);
        xact[kSideObias * kActMaxA + aa] = in ? p.obias[aa] : 0.0f;
        xact[kSideSigma * kActMaxA + aa] = c.s;
        xact[kSideLs * kActMaxA + aa] = c.ls;
        xact[kSideInvDen * kActMaxA + aa] = c.inv_den;
        xact[kSideInvS * kActMaxA + aa] = c.inv_s;
        xact[kSideInvS3 * kActMaxA + aa] = c.inv_s3;
        xact[kSideKlOs * kActMaxA + aa] = f.os;
        xact[kSideKlT1 * kActMaxA + aa] = f.t1;
        xact[kSideKlD * kActMaxA + aa] = f.D;
        xact[kSideKlRD * kActMaxA + aa] = f.rD;
        float ent = 0.0f;
#pragma unroll
        for (int b = 0; b < kActMaxA; ++b) {
            const float lb = __shfl(c.ls, b, kWave);  // lanes 0..15 of this wave are all here
            if (b < A) ent = __fadd_rn(ent, entropy_term(lb));
        }
        if (aa == 0) xact[kSideEnt * kActMaxA] = ent;
    }
    {
        float4 v[8];
        kh_load_x(p.a, static_cast<int64_t>(t_begin) * kKhT, v);
        kh_store_x(v, lds);
    }
    // W_out[o][c] of the column walk = the sum of the transposed image's three planes (exact: they were split from it)
    float wcol[QA];
#pragma unroll
    for (int lh = 0; lh < (QA + 7) / 8; ++lh) {
        uint4 q3[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) q3[pl] = ap.w_t_img[(pl * kX6PlaneB + swz(tl.c, lh)) / 16];
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
    __syncthreads();

    // the loss: row rl of the tile on lanes q = 0..3, slots a0 .. a0 + APL - 1; a slot past A works on action A - 1's
    // data (finite, in bounds), adds to no sum, stores nothing to global memory and writes an exact 0 into the d mu tile
    const int rl = t >> 2, q = t & 3, a0 = APL * q;
    bool ok[APL];
    int ak[APL];
#pragma unroll
    for (int k = 0; k < APL; ++k) {
        ok[k] = a0 + k < A;
        ak[k] = min(a0 + k, A - 1);
    }
    auto cst = [&](int r, int aa) { return xact[r * kActMaxA + aa]; };
    const uint4* oimg = p.oimg + tl.wn * (2 * 2 * 3 * 64);
    float wacc[QA];
#pragma unroll
    for (int o = 0; o < QA; ++o) wacc[o] = 0.f;
    float dbsum = 0.f;  // wave 0, lane (o, quarter): d mu column o

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t row0 = static_cast<int64_t>(tile) * kKhT;
        const bool has_next = tile + 1 < t_end;
        f32x16 acc[2];
        tl.main_loop(acc);
        // the row's loss operands: wave-uniform bases and 32-bit element offsets
        const int64_t row = row0 + rl, tile0 = row0 * A;
        const uint32_t e0 = static_cast<uint32_t>(rl * A);
        float x[APL], om[APL], os[APL];
#pragma unroll
        for (int k = 0; k < APL; ++k) {
            x[k] = (ap.actions + tile0)[e0 + ak[k]];
            om[k] = (ap.old_mu + tile0)[e0 + ak[k]];
            os[k] = (ap.old_sigma + tile0)[e0 + ak[k]];
        }
        const float old_logp = ap.old_logp[row], adv = ap.adv[row], V = ap.values[row], tv = ap.target_values[row],
                    R = ap.returns[row];
        kh_barrier();  // every wave has read the x planes: the stage takes them over
        // ---- H and the output layer's partial tile (the forward's NR = 4 epilogue: the same MFMAs in the same order)
        if (tl.live) {
            tl.elu_bias(acc, side);
            f32x16 oacc = f32x16{};
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 vb[3], wa[3];
                    uint2 lo[3], hi[3];
                    split4(make_float4(acc[j][8 * s2], acc[j][8 * s2 + 1], acc[j][8 * s2 + 2], acc[j][8 * s2 + 3]), lo[0],
                           lo[1], lo[2]);
                    split4(make_float4(acc[j][8 * s2 + 4], acc[j][8 * s2 + 5], acc[j][8 * s2 + 6], acc[j][8 * s2 + 7]),
                           hi[0], hi[1], hi[2]);
#pragma unroll
                    for (int qq = 0; qq < 3; ++qq) {
                        vb[qq] = __builtin_bit_cast(bf16x8, make_uint4(lo[qq].x, lo[qq].y, hi[qq].x, hi[qq].y));
                        wa[qq] = __builtin_bit_cast(bf16x8, oimg[((j * 2 + s2) * 3 + qq) * 64 + lane]);
                    }
                    oacc = mfma_x6(wa, vb, oacc);
                    __builtin_amdgcn_sched_barrier(0);  // one k step at a time: its planes die before the next split
                }
            float* rd = red + (tl.ib * 2 + tl.wn) * kRed;
#pragma unroll
            for (int r = 0; r < 8; ++r) rd[((r & 3) + 8 * (r >> 2) + 4 * tl.h) * 32 + tl.l32] = oacc[r];
            tl.stage_h(acc, stg);
        }
        // the next tile's x into the registers H has just left: it lands behind the loss and the column walk
        float4 vn[8];
        if (has_next) kh_load_x(p.a, row0 + kKhT, vn);
        kh_barrier();  // the partial tiles and the stage complete
        // ---- mu and the loss of the row (actor_head_any_epilogue's phase 2 on this tile's 64 rows)
        float mu[APL];
#pragma unroll
        for (int k = 0; k < APL; ++k) {
            const float* b = red + (rl >> 5) * 2 * kRed + ak[k] * 32 + (rl & 31);
            // linear_fwd_out_ex's ((p0 + p1) + p2) + p3: the partials of the wave columns past N are exact zeros
            const float p1 = NW == 2 ? b[kRed] : 0.f;
            const float sum = ((b[0] + p1) + 0.f) + 0.f;
            mu[k] = sum + cst(kSideObias, ak[k]);
            if (ok[k]) (p.y + tile0)[e0 + ak[k]] = mu[k];
        }
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
        // the value loss term only: its gradient is the critic head's, so g_value is unused
        (void)value_loss(V, tv, R, ap.clipped_value, ap.clip, 0.0f, vterm);
#pragma unroll
        for (int k = 0; k < APL; ++k) {
            float gm, gs;
            normal_grads(d[k], cst(kSideInvDen, ak[k]), cst(kSideInvS, ak[k]), cst(kSideInvS3, ak[k]), gj, ap.g_ent, gm,
                         gs);
            dmu[rl * 16 + a0 + k] = ok[k] ? gm : 0.0f;
            if (ap.grad_mu && ok[k]) (ap.grad_mu + tile0)[e0 + ak[k]] = gm;
            double v = static_cast<double>(ok[k] ? gs : 0.0f);  // d sigma: the wave's rows of slot k, per quad lane
#pragma unroll
            for (int off = 4; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
            if (lane < 4 && APL * lane + k < A) wstat[tl.wave * kWs + 4 + APL * lane + k] += v;
        }
        if (q == 3) {
#pragma unroll
            for (int c4 = APL; c4 < 4; ++c4)
                *reinterpret_cast<float4*>(dmu + rl * 16 + 4 * c4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        {
            const double s0 = wave_sum(static_cast<double>(q == 0 ? sterm : 0.0f));
            const double s1 = wave_sum(static_cast<double>(q == 0 ? vterm : 0.0f));
            const double s2 = wave_sum(static_cast<double>(q == 0 ? ent_shared : 0.0f));
            const double s3 = wave_sum(static_cast<double>(ap.compute_kl ? klpart : 0.0f));
            if (lane == 0) {
                wstat[tl.wave * kWs + 0] += s0;
                wstat[tl.wave * kWs + 1] += s1;
                wstat[tl.wave * kWs + 2] += s2;
                wstat[tl.wave * kWs + 3] += s3;
            }
        }
        kh_barrier();  // the d mu tile complete
        // ---- the output layer's backward
        if (tl.wave == 0) {  // db: lane (o, quarter) adds its 16 rows of d mu column o in order, then the quarters
            const int o = lane & 15, part = lane >> 4;
            float s = 0.f;
#pragma unroll 8
            for (int r = 16 * part; r < 16 * part + 16; ++r) s += dmu[r * 16 + o];
            s += __shfl_xor(s, 16, kWave);
            s += __shfl_xor(s, 32, kWave);
            dbsum += s;
        }
#pragma unroll 4
        for (int l = 0; l < T::kRPG; ++l) {
            const int r = T::kRPG * tl.rg + l;
            float* hp = stg + kh_stage_idx<kN>(r, tl.c >> 2) + (tl.c & 3);
            const float hv = *hp;
            const float4* dr = reinterpret_cast<const float4*>(dmu + r * 16);
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
        tl.store_dz(stg, p.c, row0, p.nt);
        __syncthreads();  // the stage and the d mu tile are read: the next tile's planes (or the dW row groups) take the LDS
        if (has_next) {
            kh_store_x(vn, lds);
            __syncthreads();
        }
    }
    // ---- the slice's partial row [dW (A x N) | db (A) | 0 pad]: the row groups in order through LDS [rg][o][N]
#pragma unroll
    for (int o = 0; o < QA; ++o) stg[(tl.rg * QA + o) * kN + tl.c] = wacc[o];
    __syncthreads();
    float* wp = ap.wpart + static_cast<int64_t>(blockIdx.x) * act_tile_floats(A, kN);
    for (int idx = t; idx < A * kN; idx += kKhThreads) {
        const int o = idx / kN, c = idx - o * kN;
        float v = stg[o * kN + c];
#pragma unroll
        for (int g = 1; g < T::kRG; ++g) v += stg[(g * QA + o) * kN + c];
        wp[idx] = v;
    }
    if (t < ((A + 3) & ~3)) wp[A * kN + t] = t < A ? dbsum : 0.f;  // thread t < 16: wave 0, lane (o = t, quarter 0)
    double v = 0.0;
    if (t < cols) {
        v = wstat[t];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += wstat[w * kWs + t];
    }
    if (fold_grid_partials<kActMaxCols>(ap.partials, ap.tickets, static_cast<int>(gridDim.x), cols, v, folded, flag)) {
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

template <int NW>
void launch_actor_head_k128(int A, dim3 g, hipStream_t st, const KhArgs& k, const ActorParams& ap) {
    const dim3 b(kKhThreads);
    if (A <= 8) hipLaunchKernelGGL((actor_head_k128_kernel<2, NW>), g, b, 0, st, k, ap);
    else if (A <= 12) hipLaunchKernelGGL((actor_head_k128_kernel<3, NW>), g, b, 0, st, k, ap);
    else hipLaunchKernelGGL((actor_head_k128_kernel<4, NW>), g, b, 0, st, k, ap);
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int64_t rslrl_head_k128_partial_rows(int64_t M) { return M >= kKhT && M % kKhT == 0 ? kh_slices(M) : 0; }

extern "C" size_t rslrl_actor_head_k128_workspace_bytes(int64_t M) {
    const int64_t s = M > 0 ? kh_slices(ceil_div(M, kKhT) * kKhT) : 0;
    return 1024 + sizeof(double) * static_cast<size_t>(kActMaxCols * (s + ceil_div(s, kFoldGroup)));
}

extern "C" int rslrl_value_head_fwd_bwd_k128(const rslrl_linear_args_t* a, const rslrl_value_head_args_t* v,
                                             rslrl_stream_t stream) {
    if (!a || !v || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    if (!kh_shape_ok(a)) return RSLRL_E_UNSUPPORTED;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    if (a->nout != 1 || v->colsum_partials) return RSLRL_E_UNSUPPORTED;
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
    const KhArgs k = kh_args(a, p);
    const dim3 g(static_cast<unsigned>(kh_slices(a->M))), b(kKhThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (a->N == 64) hipLaunchKernelGGL(value_head_k128_kernel<1>, g, b, 0, st, k);
    else hipLaunchKernelGGL(value_head_k128_kernel<2>, g, b, 0, st, k);
    return launch_status();
}

extern "C" int rslrl_actor_head_fwd_bwd_k128(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h,
                                             void* workspace, size_t workspace_bytes, rslrl_stream_t stream) {
    if (!a || !h || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    if (!kh_shape_ok(a)) return RSLRL_E_UNSUPPORTED;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    const int A = a->nout;
    if (A < kActMinA || A > kActMaxA || h->num_actions != A) return RSLRL_E_UNSUPPORTED;
    ActorParams ap{};
    const int prc = actor_head_params(a, h, workspace, workspace_bytes, ap,
                                      rslrl_actor_head_k128_workspace_bytes(a->M), kl_fast_enabled());
    if (prc) return prc;
    const KhArgs k = kh_args(a, p);
    const dim3 g(static_cast<unsigned>(kh_slices(a->M)));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (a->N == 64) launch_actor_head_k128<1>(A, g, st, k, ap);
    else launch_actor_head_k128<2>(A, g, st, k, ap);
    return launch_status();
}
