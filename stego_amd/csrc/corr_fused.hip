// Host side of the fused forward (the kernel, and why it is one launch: corr_fused_kernel.h): what it covers, the workspace hand-off words,
// the launch geometry, the choice between the full-tile and the column-half launch, and the even-K instantiations of C = 384 / 768.
#include "corr_fused_kernel.h"
#include "launchers.h"

namespace stego {

bool fused_supported(const FusedParams& prm, int precision)
{
    auto cl4 = [&](const MapV& m) {
        return m.sc == 1 && (m.sn % 4) == 0 && (m.sh % 4) == 0 && (m.sw % 4) == 0 &&
               (reinterpret_cast<uintptr_t>(m.p) % 16) == 0 &&
               ((long long)(prm.H - 1) * m.sh + (long long)(prm.W - 1) * m.sw + prm.C) * 4 < (1ll << 31);
    };
    auto cl2 = [&](const MapV& m) {          // channels-last code map; 4-byte aligned pixels are enough (odd K), K >= 3 then (see code_loads)
        return m.sc == 1 && (reinterpret_cast<uintptr_t>(m.p) % 4) == 0;
    };
    if (!(prm.C == 192 || prm.C == 384 || prm.C == 768)) return false;         // NJ instantiations below (ViT-T / ViT-S / ViT-B)
    // One workgroup per compute unit at a time (136 KB of LDS): the in-launch hand-offs (anchors, old_mean) are between workgroups
    // that run at the same time.  More tiles than CUs run as rounds of whole pair-sets (see the kernel), so a pair-set must fit:
    if (prm.B > (device_cu_count() & ~7)) return false;                       // (one pair-set = B tiles per round at least)
    if (!cl4(prm.feats) || !cl4(prm.feats_pos) || !cl2(prm.code) || !cl2(prm.code_pos)) return false;
    if (prm.K > 128 || (prm.K % 2 != 0 && prm.K < 3)) return false;             // four code K-chunks of <= 32 channels
    if (prm.H > 256 || prm.W > 256) return false;                             // packed tap coordinates (8 bits each)
    if ((long long)(prm.H - 1) * prm.code.sh + (long long)(prm.W - 1) * prm.code.sw + prm.K >= (1ll << 29)) return false;
    if ((long long)(prm.H - 1) * prm.code_pos.sh + (long long)(prm.W - 1) * prm.code_pos.sw + prm.K >= (1ll << 29)) return false;
    (void)precision;
    return true;
}

// Zeroes the hand-off words of a workspace (once per workspace; every launch leaves them zero again).
hipError_t prepare_corr_fused(const FusedParams& prm, size_t sync_bytes, hipStream_t stream)
{
    return hipMemsetAsync(prm.anchor_cnt, 0, sync_bytes, stream);
}

// The column-half launch (corr_fused_half.hip): small batches - every column half of every tile gets a compute unit of its own (16 B <= CUs
// with five negatives: the reference's batch size of 16), the device is ours alone, the BASELINE widths with an even code dimension, more
// than 64 sample points (below that the second half would be padding).  Any STEGO_DEBUG bit but the stamps (256) keeps the full-tile
// kernel - its ablation / forced-path bits mean that kernel; bit 16384 has no other meaning: same-process A/B of the two launches.
static bool half_launch_covers(const FusedParams& prm, bool shared, int all, int* n_anchor_wg)
{
    if (shared || (prm.debug & ~(256 | 7)) != 0 || !prm.rowg) return false;       // (1: timing ablation of the half kernel - no MFMA; 2: its twelve-wave form; 4: the closing ticket at the end)
    if (!(prm.C == 384 || prm.C == 768) || (prm.K & 1) || prm.P <= 64) return false;
    const int n_items = 2 * prm.n_sets * prm.B;
    if (n_items + 8 > all) return false;
    *n_anchor_wg = (all - n_items) & ~7;
    return true;
}

static hipError_t launch_fused_even(const FusedParams& prm, int precision, dim3 grid, dim3 block, int lds, hipStream_t stream)
{
    return prm.C == 384 ? launch_fused_nkc<3, false, false, 1, 2, 3, 4>(prm, precision, grid, block, lds, stream)
                        : launch_fused_nkc<6, false, false, 1, 2, 3, 4>(prm, precision, grid, block, lds, stream);
}

hipError_t launch_corr_fused(const FusedParams& prm_in, int precision, size_t sync_bytes, bool prepared, bool shared_device,
                             hipStream_t stream, hipEvent_t* ev /* null or [4]: before the memset, before / after the kernel, end */)
{
    FusedParams prm = prm_in;
    const int n_tiles = prm.n_sets * prm.B;
    const int cus = device_cu_count();
    // Every CU gets a workgroup: those beyond the tiles only help with phase 1.  That needs the WHOLE device at once; when other
    // kernels run beside the loss (STEGO_SHARED_DEVICE: the gradient all-reduce of step t overlaps the forward of step t + 1), a
    // helper that cannot be placed would hold up its anchors - and their 7 tiles each - for as long as the other kernel runs.
    // Then the tiles' own workgroups share phase 1 (a third of them take a second pass) and the CUs beyond the tiles stay free.
    const int all = (cus & ~7) < 8 ? 8 : (cus & ~7);
    // rounds of whole pair-sets: as many as fit the compute units at once (all 2 + n_neg of them when n_tiles <= CUs)
    prm.ps_round = all / prm.B < 1 ? 1 : (all / prm.B > prm.n_sets ? prm.n_sets : all / prm.B);
    const int sd = shared_device ? 1 : knob(KNOB_SHARED_DEVICE);       // (the knob: tools only - a per-call setting is a descriptor flag)
    prm.n_owner = sd == 0 ? all : (n_tiles < all ? n_tiles : all);
    if (sd > 8) {                          // (tools: an explicit number of phase-1 owners between the two, a multiple of 8)
        const int want = sd & ~7;
        prm.n_owner = want < prm.n_owner ? prm.n_owner : (want > all ? all : want);
    }
    // phase 1 carried by the light workgroups (see the kernel): one round, whole images per XCD, a workgroup on every CU, and what the
    // light ones cannot take fits one pass (16 rows at C = 384, 8 at 768) of the others
    {
        const int G = prm.C <= 384 ? 2 : 1, rowsL = 24 * G + ((prm.C <= 384 && !(prm.debug & 2048)) ? 16 : 0), rowsH = 8 * G;
        const int per_x = prm.B / 8, slots = all / 8, tile_slots = n_tiles / 8;
        const int n_light = per_x + (slots - tile_slots), n_heavy = slots - n_light;
        const int R = per_x * TP, rest = R - n_light * rowsL;
        prm.p1_light = !(prm.debug & 128) && prm.B % 8 == 0 && n_tiles % 8 == 0 && n_tiles <= all && prm.n_owner == all && prm.ps_round >= prm.n_sets &&
                       slots >= tile_slots && n_light > 0 && (rest <= 0 || (n_heavy > 0 && (rest + n_heavy - 1) / n_heavy <= rowsH)) ? 1 : 0;
    }
    prm.timeout_ticks = 20000;                                    // 200 us of the 100 MHz clock (debug 64: the anchor wait gives up after 1 us)
    const int lds = RING_LDS_BYTES;
    hipError_t e = hipSuccess;
    if (ev) (void)hipEventRecord(ev[0], stream);
    if (!prepared && (e = prepare_corr_fused(prm, sync_bytes, stream)) != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], stream);
    if (half_launch_covers(prm, sd != 0, all, &prm.n_anchor_wg)) {
        if ((e = launch_fused_half(prm, precision, stream)) != hipSuccess) return e;      // (the runtime's answer to the launch included)
        if (ev) { (void)hipEventRecord(ev[2], stream); (void)hipEventRecord(ev[3], stream); }
        return hipGetLastError();
    }
    const dim3 grid(n_tiles > prm.n_owner ? n_tiles : prm.n_owner), block(FUSED_THREADS);
    e = prm.C == 192 ? launch_fused_c192(prm, precision, grid, block, lds, stream)
        : (prm.K & 1) ? launch_fused_odd(prm, precision, grid, block, lds, stream) : launch_fused_even(prm, precision, grid, block, lds, stream);
    if (e != hipSuccess) return e;
    if (ev) { (void)hipEventRecord(ev[2], stream); (void)hipEventRecord(ev[3], stream); }
    return hipGetLastError();
}

}  // namespace stego
