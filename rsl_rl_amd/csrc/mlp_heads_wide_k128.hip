// The fused actor head for 17 to 32 actions on a last hidden layer with 128 inputs (Linear(128, N) + ELU + the output
// Linear, N = 64 or 128: the tails of [128, 128, 128], [256, 128, 128] and [256, 128, 64] at H1 flat's 19 actions and
// its like): the last hidden layer, the output layer, the whole PPO loss and the output layer's backward in one launch.
//   rslrl_actor_head_wide_fwd_bwd_k128   actor: mu, the PPO loss and its statistics, d mu, d sigma, dZ, [dW | db] partials
// The contract is the wide head's (mlp_head_wide.hip: mu with linear_fwd_out_ex's bits, d mu with ppo_loss_kernel<32>'s,
// dZ on the x6 MFMA), the geometry the 128-input heads' (heads_k128_tile.h, described in mlp_heads_k128.hip): 4 waves,
// a 64-row tile whose x stays in LDS as three bf16 planes, weight fragments from L2, two workgroups per CU, each
// walking a slice of consecutive tiles and writing one partial row and one column of loss partials per slice.
//
// Per tile, wave (ib, wn) on rows [32 ib, 32 ib + 32) and H columns [64 wn, 64 wn + 64) (at N = 64 the wn = 1 waves
// hold no column: they skip the MFMAs, reach every barrier and take their share of everything else):
//  1. KhTile::main_loop; the loss inputs of the thread's two rows are requested.                            barrier
//  2. H = ELU(acc + b); the output layer as one 32 x 32 x6 MFMA block per wave (the forward's NR = 4 epilogue: the same
//     MFMAs in the same order, all 16 accumulator registers) -> red [ib][wn][32 outputs][32 rows]; H into the stage;
//     the next tile's x is requested into the registers H has left.                                        barrier
//  3. the loss in two turns of 32 rows (turn u = the rows of the ib = u waves): row 32 u + (t >> 3) on the octet's
//     lanes q = t & 7, actions 4 q .. 4 q + 3 below A.  mu = ((p0 + p1) + 0) + 0 + bias -- linear_fwd_out_ex's
//     four-term sum, whose terms past N are exact zeros.  ppo_loss_common.h's expressions on the per-action rows of
//     the side area; the log-prob is tree_sum<32>'s sum (the lane's four terms as a running sum, then octet_sum).
//     -> the d mu tile [64][32] (a slot past A works on action A - 1, adds to no sum, stores nothing to global
//     memory and writes an exact +0); each wave adds its fp64 loss sums to its own wstat row in LDS.          barrier
//  4. db: wave 0, lane (o, half) adds its 32 rows of d mu column o in row order in fp64, then the halves; kept in
//     fp64 across the slice and rounded once, into the slice's partial row.  dW: thread (column c, action group ag
//     of 16[, row group]) walks column c of the staged rows with the d mu row broadcast from LDS: 16 accumulators
//     kept across the slice (N = 128: 128 columns x 2 groups x 64 rows; N = 64: 64 columns x 2 groups x 2 row groups
//     of 32, added in order through LDS at the slice's end).                                                barrier
//  5. dZ = (d mu W_out) * ELU'(H): per live wave two 32 x 32 blocks of two 16-deep x6 MFMA k steps on the W_out^T image
//     (L2; zero from k = A on) and the split d mu rows; H comes back from the stage and dZ replaces it in place, then
//     leaves as 256-byte row segments (KhTile::store_dz; at N = 64 behind one more barrier: its regions are 16 rows of
//     every wave).                                                                                          barrier
//  6. the next tile's x is split into the planes.                                                           barrier
// LDS (59.4 KiB): [0, 48K) the x planes; once the main loop is done [0, 4 * 64 N) is the H stage and [32K, 48K) -- plane
// bytes the stage never reaches -- the partial tiles red; at the slice's end [0, 16K) holds N = 64's dW row groups.
// [48K, 59.4K) the side area: hidden bias [128], kActSideRows per-action rows of 32, the d mu tile (8 KiB, float4 quads
// XOR-swizzled by row & 7), then fp64: wstat [4 waves][36], folded [36], the flag.
#include "actor_head_host.h"
#include "common.h"
#include "heads_k128_tile.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

constexpr int kKwA = kActWideMaxA;                     // the padded width: side-row stride, d mu columns
constexpr int kKwCols = kActWideCols;                  // loss partial columns: surrogate, value, entropy, KL, d sigma [32]
constexpr int kKwRedTile = kKwA * 32;                  // floats of one (ib, wn) partial tile
constexpr int kKwRedB = kKhXBytes - 4 * 4 * kKwRedTile;  // red: the last 16 KiB of the plane area
// side area (floats from kKhXBytes)
constexpr int kKwAct = 128;                            // behind the hidden bias: kActSideRows rows of kKwA
constexpr int kKwDmu = kKwAct + kActSideRows * kKwA;   // d mu [64][32]
constexpr int kKwStat = kKwDmu + kKhT * kKwA;          // fp64: wstat [4 waves][kKwCols], folded [kKwCols], flag
constexpr int kKwSideBytes = 4 * kKwStat + 8 * (5 * kKwCols) + 16;
constexpr int kKwLds = kKhXBytes + kKwSideBytes;
constexpr int kKwDwA = 16;                             // actions per dW thread group
static_assert(kKwRedB >= 4 * kKhT * 128, "wide k128 head: red behind the widest H stage");
static_assert(2 * kKwA * 64 * 4 <= kKhXBytes, "wide k128 head: N = 64's dW row groups in the plane area");
static_assert(kKwLds <= 80 * 1024, "wide k128 head: two workgroups per CU");
static_assert((4 * kKwStat) % 8 == 0 && (4 * kKwDmu) % 16 == 0, "wide k128 head: fp64 loss partials, float4 d mu");
static_assert(2 * kKwDwA == kKwA && 4 * kKwCols <= kKhThreads, "wide k128 head: two dW action groups, wstat's zeroing");

// red: the row index XORed with 8 ((o >> 2) & 3) (the loss's reads of four actions per lane spread over the banks);
// d mu: float4 quads XOR-swizzled by row & 7 (the dZ fragment reads walk rows at a stride of 32 floats)
__device__ __forceinline__ int kw_red_idx(int o, int r) { return o * 32 + (r ^ (((o >> 2) & 3) << 3)); }
__device__ __forceinline__ int kw_dmu_idx(int r, int quad) { return r * kKwA + 4 * (quad ^ (r & 7)); }

template <int NW>
__global__ __launch_bounds__(kKhThreads, 2) void actor_head_wide_k128_kernel(KhArgs a, ActorParams ap) {
    using T = KhTile<NW>;
    constexpr int kN = T::kN;
    constexpr int kW = kKwA, kRed = kKwRedTile, kWs = kKwCols;
    constexpr int kDwRG = 2 / NW;       // row groups of the dW walk
    constexpr int kDwRows = kKhT / kDwRG;
    __shared__ __attribute__((aligned(16))) char lds[kKwLds];
    const GemmParams& p = a.p;
    float* const stg = reinterpret_cast<float*>(lds);
    float* const red = reinterpret_cast<float*>(lds + kKwRedB);
    float* const side = reinterpret_cast<float*>(lds + kKhXBytes);
    float* const xact = side + kKwAct;
    float* const dmu = side + kKwDmu;
    double* const wstat = reinterpret_cast<double*>(side + kKwStat);  // [4 waves][kWs]
    double* const folded = wstat + 4 * kWs;
    int* const flag = reinterpret_cast<int*>(folded + kWs);
    T tl;
    tl.init(lds, a.img);
    const int t = threadIdx.x, lane = tl.lane;
    const int A = p.nout;  // wave-uniform
    const int cols = 4 + A;
    const int t_begin = blockIdx.x * a.tiles_per;
    const int t_end = min(a.tiles, t_begin + a.tiles_per);

    // ---- once per slice: the waves' loss sums, the bias, the per-action rows (lane a of the last wave: sigma_consts and
    // kl_fast_consts of action a, of sigma 1 past A, and the entropy of a row), the first x tile
    if (t < 4 * kWs) wstat[t] = 0.0;
    if (t < kN / 4) reinterpret_cast<float4*>(side)[t] = *reinterpret_cast<const float4*>(p.bias + 4 * t);
    if (t >= kKhThreads - kWave && t < kKhThreads - kWave + kW) {
        const int aa = t - (kKhThreads - kWave);
        const bool in = aa < A;
        const SigmaConsts c = sigma_consts(in ? ap.sigma[aa] : 1.0f);
        const KlFastConsts f = kl_fast_consts(c.s, in ? ap.old_sigma[aa] : 1.0f, ap.kl_fast);
        xact[kSideObias * kW + aa] = in ? p.obias[aa] : 0.0f;
        xact[kSideSigma * kW + aa] = c.s;
        xact[kSideLs * kW + aa] = c.ls;
        xact[kSideInvDen * kW + aa] = c.inv_den;
        xact[kSideInvS * kW + aa] = c.inv_s;
        xact[kSideInvS3 * kW + aa] = c.inv_s3;
        xact[kSideKlOs * kW + aa] = f.os;
        xact[kSideKlT1 * kW + aa] = f.t1;
        xact[kSideKlD * kW + aa] = f.D;
        xact[kSideKlRD * kW + aa] = f.rD;
        float ent = 0.0f;
#pragma unroll
        for (int b = 0; b < kW; ++b) {
            const float lb = __shfl(c.ls, b, kWave);  // lanes 0..31 of this wave are all here
            if (b < A) ent = __fadd_rn(ent, entropy_term(lb));
        }
        if (aa == 0) xact[kSideEnt * kW] = ent;
    }
    {
        float4 v[8];
        kh_load_x(p.a, static_cast<int64_t>(t_begin) * kKhT, v);
        kh_store_x(v, lds);
    }
    __syncthreads();

    // the loss: row 32 u + hr of the tile in turn u, on lanes q = 0..7, actions a0 .. a0 + 3 below A; a masked slot works
    // on the last action's data (finite, in bounds) and stores and adds nothing
    const int hr = t >> 3, q = t & 7, a0 = 4 * q;
    bool ok[4];
    int ak[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = a0 + k < A;
        ak[k] = min(a0 + k, A - 1);
    }
    auto cst = [&](int r, int aa) { return xact[r * kW + aa]; };
    // the output layer's fragments (this wave column's 12 KiB of the output image) and W_out^T's (two 16-action chunks)
    // through buffer resources: one lane offset each, the fragment's place as an immediate -- 64-bit addresses per
    // fragment, hoisted out of the tile loop, were the first thing the register allocator spilled
    const __amdgpu_buffer_rsrc_t roimg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4*>(p.oimg + tl.wn * (2 * 2 * 3 * 64)), 0, 2 * 2 * 3 * 64 * 16, kKhRsrcFlags);
    const __amdgpu_buffer_rsrc_t rwt =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(ap.w_t_img), 0, 2 * kX6ChunkB, kKhRsrcFlags);
    // the backward: dW column c, actions kKwDwA ag .., rows [kDwRows drg, kDwRows drg + kDwRows) (ag, drg wave-uniform)
    const int c = t & (kN - 1), ag = (t / kN) & 1, drg = t / (2 * kN);
    float wacc[kKwDwA];
#pragma unroll
    for (int o = 0; o < kKwDwA; ++o) wacc[o] = 0.f;
    double dbs = 0.0;  // wave 0: db of column lane & 31 (both halves of the lanes hold the sum)

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t row0 = static_cast<int64_t>(tile) * kKhT;
        const bool has_next = tile + 1 < t_end;
        f32x16 acc[2];
        tl.main_loop(acc);
        // the rows' loss operands: wave-uniform bases and 32-bit element offsets
        const int64_t tile0 = row0 * A;
        float x[2][4], om[2][4], os[2][4], old_logp[2], adv[2], V[2], tv[2], R[2];
        auto load_row = [&](int u) {  // turn u's row: 32 u + hr
            const int rl = 32 * u + hr;
            const uint32_t e0 = static_cast<uint32_t>(rl * A);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[u][k] = (ap.actions + tile0)[e0 + ak[k]];
                om[u][k] = (ap.old_mu + tile0)[e0 + ak[k]];
                os[u][k] = (ap.old_sigma + tile0)[e0 + ak[k]];
            }
            old_logp[u] = ap.old_logp[row0 + rl];
            adv[u] = ap.adv[row0 + rl];
            V[u] = ap.values[row0 + rl];
            tv[u] = ap.target_values[row0 + rl];
            R[u] = ap.returns[row0 + rl];
        };
        load_row(0);
        kh_barrier();  // every wave has read the x planes: the stage and red take them over
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
                        wa[qq] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                                                roimg, 16 * lane, ((j * 2 + s2) * 3 + qq) * 1024, 0));
                    }
                    oacc = mfma_x6(wa, vb, oacc);
                    __builtin_amdgcn_sched_barrier(0);  // one k step at a time: its planes die before the next split
                }
            float* rd = red + (tl.ib * 2 + tl.wn) * kRed;
#pragma unroll
            for (int r = 0; r < 16; ++r) rd[kw_red_idx((r & 3) + 8 * (r >> 2) + 4 * tl.h, tl.l32)] = oacc[r];
            tl.stage_h(acc, stg);
        }
        // the next tile's x into the registers H has just left: it lands behind the loss and the backward
        float4 vn[8];
        if (has_next) kh_load_x(p.a, row0 + kKhT, vn);
        load_row(1);   // the second turn's row lands behind the first turn's loss
        kh_barrier();  // the partial tiles and the stage complete
        // ---- mu and the loss of the thread's two rows
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rl = 32 * u + hr;
            const uint32_t e0 = static_cast<uint32_t>(rl * A);
            float mu[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* b = red + u * 2 * kRed + kw_red_idx(ak[k], hr);
                // linear_fwd_out_ex's ((p0 + p1) + p2) + p3: the partials of the wave columns past N are exact zeros
                const float p1 = NW == 2 ? b[kRed] : 0.f;
                const float sum = ((b[0] + p1) + 0.f) + 0.f;
                mu[k] = sum + cst(kSideObias, ak[k]);
                if (ok[k]) (p.y + tile0)[e0 + ak[k]] = mu[k];
            }
            float d[4], lsum = 0.0f, klpart = 0.0f;
            bool kl_slow = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d[k] = x[u][k] - mu[k];
                const float term = logp_term(d[k], cst(kSideInvDen, ak[k]), cst(kSideLs, ak[k]));
                // tree_sum: a running sum inside the lane's block of four, entries from A on count as 0
                lsum = k == 0 ? (ok[0] ? term : 0.0f) : __fadd_rn(lsum, ok[k] ? term : 0.0f);
                const KlFastConsts kf = {cst(kSideKlOs, ak[k]), cst(kSideKlT1, ak[k]), cst(kSideKlD, ak[k]),
                                         cst(kSideKlRD, ak[k])};
                bool slow = false;
                const float kt = kl_term_fast(kf, os[u][k], mu[k], om[u][k], slow);
                if (ok[k]) {
                    klpart = __fadd_rn(klpart, kt);
                    kl_slow |= slow;
                }
            }
            if (ap.compute_kl && kl_slow) {  // the reference's exact expression for every element of this lane (rare)
                klpart = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float kt = kl_term_exact(cst(kSideSigma, ak[k]), os[u][k], mu[k], om[u][k]);
                    if (ok[k]) klpart = __fadd_rn(klpart, kt);
                }
            }
            const float ent_shared = cst(kSideEnt, 0);
            const float logp = octet_sum(lsum);  // then the tree over the eight blocks, strides 1, 2, 4
            float gj, vterm;
            const float sterm = surrogate(logp, old_logp[u], adv[u], ap.ratio_lo, ap.ratio_hi, ap.g_surr, gj);
            // the value loss term only: its gradient is the critic head's, so g_value is unused
            (void)value_loss(V[u], tv[u], R[u], ap.clipped_value, ap.clip, 0.0f, vterm);
            float gsg[4], gmv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float gm, gs;
                normal_grads(d[k], cst(kSideInvDen, ak[k]), cst(kSideInvS, ak[k]), cst(kSideInvS3, ak[k]), gj, ap.g_ent,
                             gm, gs);
                gsg[k] = ok[k] ? gs : 0.0f;
                gmv[k] = ok[k] ? gm : 0.0f;
                if (ap.grad_mu && ok[k]) (ap.grad_mu + tile0)[e0 + ak[k]] = gm;
            }
            *reinterpret_cast<float4*>(dmu + kw_dmu_idx(rl, q)) = make_float4(gmv[0], gmv[1], gmv[2], gmv[3]);
            const double s_surr = wave_sum(static_cast<double>(q == 0 ? sterm : 0.0f));
            const double s_val = wave_sum(static_cast<double>(q == 0 ? vterm : 0.0f));
            const double s_ent = wave_sum(static_cast<double>(q == 0 ? ent_shared : 0.0f));
            const double s_kl = wave_sum(static_cast<double>(ap.compute_kl ? klpart : 0.0f));
            double* ws = wstat + tl.wave * kWs;
            if (lane == 0) {
                ws[0] += s_surr;
                ws[1] += s_val;
                ws[2] += s_ent;
                ws[3] += s_kl;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // d sigma: the wave's 8 rows of slot k, per octet lane
                double v = static_cast<double>(gsg[k]);
#pragma unroll
                for (int off = 8; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
                if (lane < 8 && 4 * lane + k < A) ws[4 + 4 * lane + k] += v;
            }
        }
        kh_barrier();  // the d mu tile complete
        // ---- the output layer's backward: db and dW
        if (tl.wave == 0) {  // lane (o, part) adds rows 32 part .. 32 part + 31 of column o in order, then the two parts
            const int o = lane & 31, part = lane >> 5;
            double s = 0.0;
#pragma unroll 8
            for (int r = 32 * part; r < 32 * part + 32; ++r)
                s += static_cast<double>(dmu[kw_dmu_idx(r, o >> 2) + (o & 3)]);
            s += __shfl_xor(s, 32, kWave);
            dbs += s;
        }
#pragma unroll 4
        for (int l = 0; l < kDwRows; ++l) {  // 4 broadcast d mu reads + 1 H read per 16 FMAs
            const int r = kDwRows * drg + l;
            const float hv = stg[kh_stage_idx<kN>(r, c >> 2) + (c & 3)];
#pragma unroll
            for (int g = 0; g < kKwDwA / 4; ++g) {
                const float4 d4 = *reinterpret_cast<const float4*>(dmu + kw_dmu_idx(r, ag * 4 + g));
                wacc[4 * g] = fmaf(d4.x, hv, wacc[4 * g]);
                wacc[4 * g + 1] = fmaf(d4.y, hv, wacc[4 * g + 1]);
                wacc[4 * g + 2] = fmaf(d4.z, hv, wacc[4 * g + 2]);
                wacc[4 * g + 3] = fmaf(d4.w, hv, wacc[4 * g + 3]);
            }
        }
        kh_barrier();  // every wave's reads of the stage done: dZ replaces H in place
        // ---- dZ of the wave's two 32 x 32 blocks
        if (tl.live) {
            const int r = 32 * tl.ib + tl.l32;
            bf16x8 vb[2][3];  // the split d mu rows: k step s holds actions 16 s + 8 h .. + 7 of row r
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float4 v0 = *reinterpret_cast<const float4*>(dmu + kw_dmu_idx(r, 4 * s + 2 * tl.h));
                const float4 v1 = *reinterpret_cast<const float4*>(dmu + kw_dmu_idx(r, 4 * s + 2 * tl.h + 1));
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
                        wa[qq] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                                                rwt, tl.boff, s * kX6ChunkB + qq * kX6PlaneB + j * 32 * kX6RowB, 0));
                    dacc = mfma_x6(wa, vb[s], dacc);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float* sp = stg + kh_stage_idx<kN>(r, tl.wn * 16 + j * 8 + 2 * g + tl.h);
                    const f32x4 h4 = *reinterpret_cast<const f32x4*>(sp);
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = dacc[4 * g + e], hh = h4[e];
                        o[e] = hh > 0.f ? z : z * (hh + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
                    }
                    *reinterpret_cast<f32x4*>(sp) = o;
                }
            }
        }
        if (NW == 1) kh_barrier();  // N = 64: a wave stores 16 rows of every live wave's dZ
        tl.store_dz(stg, p.c, row0, p.nt);
        __syncthreads();  // the stage, red and the d mu tile are read: the next tile's planes (or the dW row groups) take the LDS
        if (has_next) {
            kh_store_x(vn, lds);
            __syncthreads();
        }
    }
    // ---- the slice's partial row [dW (A x N) | db (A) | 0 pad]; N = 64: the two row groups in order through LDS [drg][o][N]
    float* wp = ap.wpart + static_cast<int64_t>(blockIdx.x) * act_tile_floats(A, kN);
    if (kDwRG == 1) {
#pragma unroll
        for (int o = 0; o < kKwDwA; ++o)
            if (kKwDwA * ag + o < A) wp[(kKwDwA * ag + o) * kN + c] = wacc[o];
    } else {
#pragma unroll
        for (int o = 0; o < kKwDwA; ++o) stg[(drg * kW + kKwDwA * ag + o) * kN + c] = wacc[o];
        __syncthreads();
        for (int idx = t; idx < A * kN; idx += kKhThreads) wp[idx] = stg[idx] + stg[kW * kN + idx];
    }
    if (tl.wave == 0 && lane < ((A + 3) & ~3)) wp[A * kN + lane] = lane < A ? static_cast<float>(dbs) : 0.f;
    double v = 0.0;
    if (t < cols) {
        v = wstat[t];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += wstat[w * kWs + t];
    }
    if (fold_grid_partials<kKwCols>(ap.partials, ap.tickets, static_cast<int>(gridDim.x), cols, v, folded, flag)) {
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

}  // namespace
}  // namespace rslrl

using namespace rslrl;

// The actor head for 17 to 32 actions on a last hidden layer with 128 inputs (include/rslrl_amd.h): the wide head's
// argument structs, N = 64 or 128, M a positive multiple of 64.  Every other shape returns RSLRL_E_UNSUPPORTED before
// anything is launched.  The workspace holds the fold's tickets and 36 fp64 partial columns per slice and fold group
// (slices: rslrl_head_k128_partial_rows).
extern "C" size_t rslrl_actor_head_wide_k128_workspace_bytes(int64_t M) {
    const int64_t s = M > 0 ? kh_slices(ceil_div(M, kKhT) * kKhT) : 0;
    return 1024 + sizeof(double) * static_cast<size_t>(kKwCols * (s + ceil_div(s, kFoldGroup)));
}

extern "C" int rslrl_actor_head_wide_fwd_bwd_k128(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h,
                                                  void* workspace, size_t workspace_bytes, rslrl_stream_t stream) {
    if (!a || !h || a->op != RSLRL_LINEAR_FWD_OUT) return RSLRL_E_INVALID_ARGUMENT;
    const int A = a->nout;
    if (!kh_shape_ok(a) || A < kActWideMinA || A > kActWideMaxA || h->num_actions != A) return RSLRL_E_UNSUPPORTED;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc) return rc;
    ActorParams ap{};
    const int prc = actor_head_params(a, h, workspace, workspace_bytes, ap,
                                      rslrl_actor_head_wide_k128_workspace_bytes(a->M), kl_fast_enabled());
    if (prc) return prc;
    const KhArgs k = kh_args(a, p);
    const dim3 g(static_cast<unsigned>(rslrl_head_k128_partial_rows(a->M))), b(kKhThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (a->N == 64) hipLaunchKernelGGL(actor_head_wide_k128_kernel<1>, g, b, 0, st, k, ap);
    else hipLaunchKernelGGL(actor_head_wide_k128_kernel<2>, g, b, 0, st, k, ap);
    return launch_status();
}
