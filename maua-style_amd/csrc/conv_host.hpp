// Host launch layer shared by the convolution families (conv_x6, conv_x3, conv_x3w, conv_x3q, conv_x3p, conv_kxk_x3, conv_api): shape ->
// ConvArgs, the split-K cost model, the in-launch finish, workspace sizing and acceptance, the two-bank filter pack.  Host code only, no
// state: each family keeps its constants (a SplitModel next to its kernel) and its name in its messages.
#pragma once
#include "common.hpp"

namespace maua {

enum ConvShape { CONV_SHAPE_OK = 0, CONV_SHAPE_EMPTY, CONV_SHAPE_BAD_DIMS };

// The one place a shape becomes ConvArgs (Cin, H, W, Cout, OH, OW, pad of a k x k stride-1 convolution; everything else zero):
// conv_dims_ok BEFORE any arithmetic, an output plane without pixels afterwards.  `k` is the caller's to bound (1 ... 64).
inline ConvShape conv_geometry(ConvArgs& a, int n, int cin, int h, int w, int cout, int k, int pad) {
    a = ConvArgs{};
    if (!conv_dims_ok(n, cin, h, w, cout, pad)) return CONV_SHAPE_BAD_DIMS;
    a.Cin = cin;
    a.H = h;
    a.W = w;
    a.Cout = cout;
    a.OH = h + 2 * pad - k + 1;
    a.OW = w + 2 * pad - k + 1;
    a.pad = pad;
    return a.OH > 0 && a.OW > 0 ? CONV_SHAPE_OK : CONV_SHAPE_EMPTY;
}

// What a family's split-K decision depends on.  The policy does not look at a launch's batch size but at the number of frames the caller
// plans to evaluate per launch (maua_set_split_batch_hint, 1 by default): vid_img's frames are then computed with the same summation
// order whether they run one at a time or sixteen together - bit-identical results whatever the grouping.
struct SplitModel {
    int rows;                // a workgroup's tile: rows x 32 pixels ...
    int cot;                 // ... x cot output channels
    int chunk;               // input channels per K-loop chunk
    bool partial_chunk;      // a last chunk of fewer channels counts (the kernel pads it); else Cin is a multiple of `chunk`
    int slots;               // workgroups the chip holds at once
    int no_split_wgs;        // no split from this many workgroups ...
    int min_chunks;          // ... or below this many chunks
    int chunks_per_split;    // ks <= chunks / this
    double us_per_chunk;     // a full CU's time for one chunk
    double prologue_chunks;  // a workgroup's prologue + epilogue in chunk-times
    const char* forced;      // tuning constant that splits every launch k ways (when the layer has the chunks), or null
    bool finish_in_launch;   // the kernel can finish a split inside the launch (armed workspaces): whole-tile slabs
};

inline int64_t conv_tiles(const ConvArgs& a, int rows) { return (int64_t)((a.OW + 31) / 32) * ((a.OH + rows - 1) / rows); }
inline int64_t conv_units(const SplitModel& m, const ConvArgs& a) { return conv_tiles(a, m.rows) * ((a.Cout + m.cot - 1) / m.cot); }

// Split the K loop over several workgroups when the output grid quantises badly against the chip's workgroup slots.  Cost per candidate
// split: rounds x (chunks per workgroup + prologue) x us per chunk, plus the finish pass's traffic (ks partial reads + one write at
// ~5 TB/s: MB / 5 in us) and its launch; the smaller split unless the gain is real.  1 = no split.
inline int choose_split(const SplitModel& m, const ConvArgs& a) {
    const int64_t wgs = conv_units(m, a) * split_batch_hint();
    const int nchunks = m.partial_chunk ? (a.Cin + m.chunk - 1) / m.chunk : a.Cin / m.chunk;
    const int most = nchunks / m.chunks_per_split;
    const int forced = m.forced ? (int)tuning(m.forced, 0) : 0;
    if (forced > 0) return forced <= most ? forced : (nchunks >= m.min_chunks ? most : 1);
    if (wgs >= m.no_split_wgs || nchunks < m.min_chunks) return 1;
    const double out_mb = (double)split_batch_hint() * a.Cout * a.OH * a.OW * 4.0 / 1e6;
    int best = 1;
    double best_cost = 1e30;
    for (int ks = 1; ks <= 16 && ks <= most; ++ks) {
        const double rounds = (double)((wgs * ks + m.slots - 1) / m.slots);
        double cost = rounds * ((double)((nchunks + ks - 1) / ks) + m.prologue_chunks) * m.us_per_chunk;
        if (ks > 1) cost += (ks + 1) * out_mb / 5.0 + 5.0;
        if (cost < best_cost * 0.97) {
            best_cost = cost;
            best = ks;
        }
    }
    return best;
}

// Bytes of slabs a launch that finishes its split inside the launch needs: one slab per (image, channel tile, pixel tile, split) - whole
// tiles, so a little more than the [split][Cout][OH][OW] slabs of the two-launch form on ragged planes.
inline size_t in_launch_bytes(const SplitModel& m, const ConvArgs& a, int n, int ks) {
    return (size_t)n * ((a.Cout + m.cot - 1) / m.cot) * conv_tiles(a, m.rows) * ks * (m.cot * m.rows * 32 * 4);
}
// Whether a launch split `ks` ways finishes inside the launch: the caller armed this workspace (a.arrive), the split is small enough for
// one workgroup to add the other slabs (tuning constant finish_in_launch_max_ks, default 4), and the tiles have counters.
inline bool finish_in_launch(const SplitModel& m, const ConvArgs& a, int n, int ks) {
    return ks > 1 && a.arrive != nullptr && ks <= (int)tuning("finish_in_launch_max_ks", 4) && n * conv_units(m, a) <= ARRIVE_COUNTERS;
}

// Workspace of a launch split `ks` ways: the [n][ks][Cout][OH][OW] slabs conv_splitk_finish adds, or the whole-tile slabs of the in-launch
// finish where the family has one and they are larger (a caller that arms its workspace gets that form).
inline size_t split_workspace_bytes(const SplitModel& m, const ConvArgs& a, int n, int ks) {
    if (ks <= 1) return 0;
    const size_t two_launches = (size_t)n * ks * a.Cout * a.OH * a.OW * sizeof(float);
    const size_t in_launch = m.finish_in_launch ? in_launch_bytes(m, a, n, ks) : 0;
    return in_launch > two_launches ? in_launch : two_launches;
}

// The bodies of a family's *_split and *_workspace_bytes queries: 0 for anything that is not a shape.
inline int query_split(const SplitModel& m, int n, int cin, int h, int w, int cout, int pad) {
    ConvArgs a;
    return conv_geometry(a, n, cin, h, w, cout, 3, pad) == CONV_SHAPE_OK ? choose_split(m, a) : 0;
}
inline size_t query_workspace_bytes(const SplitModel& m, int n, int cin, int h, int w, int cout, int pad) {
    ConvArgs a;
    return conv_geometry(a, n, cin, h, w, cout, 3, pad) == CONV_SHAPE_OK ? split_workspace_bytes(m, a, n, choose_split(m, a)) : 0;
}

// The caller's workspace is the launch's if it holds need() bytes (split-K only then; without one the kernel still runs, with fewer
// workgroups, and nothing is planned: need() is not called); `arm`: and its arrival counters, if the calling thread armed this
// workspace (small splits finish inside the launch).
template <typename Need>
inline void accept_workspace(ConvArgs& a, void* workspace, size_t workspace_bytes, bool arm, Need&& need) {
    a.ws = (workspace && workspace_bytes >= need()) ? (float*)workspace : nullptr;
    a.arrive = arm && a.ws ? armed_counters(workspace) : nullptr;
}
inline void accept_workspace(ConvArgs& a, void* workspace, size_t workspace_bytes, bool arm, const SplitModel& m, int n) {
    accept_workspace(a, workspace, workspace_bytes, arm, [&] { return split_workspace_bytes(m, a, n, choose_split(m, a)); });
}

// Bytes of one direction's filter bank: [chunk][cotile] slices of `slice_bytes`.
inline size_t bank_bytes(int cout_produced, int cin_consumed, int chunk, int cot, size_t slice_bytes) {
    if (cout_produced <= 0 || cin_consumed <= 0 || cout_produced > (1 << 20) || cin_consumed > (1 << 20)) return 0;
    return (size_t)((cin_consumed + chunk - 1) / chunk) * ((cout_produced + cot - 1) / cot) * slice_bytes;
}
inline bool pack_args_ok(const float* w_oihw, const void* bank_fwd, const void* bank_bwd, int cout, int cin) {
    return w_oihw && (bank_fwd || bank_bwd) && cout > 0 && cin > 0 && cout <= (1 << 20) && cin <= (1 << 20);
}
// launch(bank, backward) packs one bank; the forward and / or the backward-data bank, each launch checked.
template <typename Launch>
inline int pack_two_banks(void* bank_fwd, void* bank_bwd, const char* kernel_name, Launch&& launch) {
    for (int backward = 0; backward < 2; ++backward) {
        void* bank = backward ? bank_bwd : bank_fwd;
        if (!bank) continue;
        launch((unsigned short*)bank, backward);
        const int rc = check_launch(kernel_name);
        if (rc) return rc;
    }
    return MAUA_OK;
}

}  // namespace maua
