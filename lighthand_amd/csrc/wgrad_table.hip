// Weight gradient, table launches: the deferred weight gradients of a whole stage as ONE grid of the LDS-DMA ring kernel
// (wgrad_ring_kernel.h: wgrad_ring_table_kernel) + (at most) ONE fold grid.  lh_wgrad_table_build plans the table on the host -- item
// length, every member's split count, the work-item order, the blob the kernels read -- and lh_wgrad_table_run launches it.
#include "wgrad_plan.h"
#include "wgrad_reduce.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <vector>

// Table launch: the folds of any number of weight gradients as one grid (items[b] = problem, block index inside it); a problem
// folds on the transposing path or the generic one (WreduceArgs.contig).  With ONE pixel split the fold is the transposition
// [tap][o][i] -> the reference layout.
__global__ __launch_bounds__(256) void wgrad_reduce_table_kernel(const WreduceArgs* __restrict__ tab, const int2* __restrict__ items) {
    extern __shared__ float tile[];
    const int2 it = items[blockIdx.x];
    const WreduceArgs& p = tab[__builtin_amdgcn_readfirstlane(it.x)];
    if (p.contig) wgrad_reduce_contig_body(p, tile, it.y);
    else wgrad_reduce_body(p, it.y, 0);
}

static inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// What the steps of lh_wgrad_table_build hand on to each other.
struct TableBuild {
    WgradPlan base;                     // the table's tile / stage / ring depth; every member gets its own split count
    long min_stages, L;                 // ring stages per work item: the floor (>= 256 pixels) and the length aimed at
    std::vector<long> stages;           // ring stages of every member
    std::vector<WgradArgs> args;        // one argument block per member
    std::vector<WreduceArgs> folds;     // the folds of the members that the kernel does not write directly
    std::vector<int2> items;            // work items in launch order: (member, block index inside it); member -1 = padding
    size_t ws = 0;                      // slab workspace
    int fold_lds = 0;
};

// Step 1: every problem's stage count; the automatic item length aims at ~4 rounds of the machine's workgroup slots.
static int table_item_length(const lh_wgrad_call* calls, int n, int target_stages, TableBuild& t) {
    const WgradPlan& base = t.base;
    const int lds = base.depth * base.kps * (base.bo + base.bi) * 2;
    const int per_cu = base.bo * base.bi >= 256 * 256 ? 1 : std::min(2, (160 * 1024) / lds);
    const long slots = 256L * per_cu;
    std::vector<long> tiles(n);
    t.stages.resize(n);
    long work = 0, smax = 0;
    for (int i = 0; i < n; ++i) {
        const lh_wgrad_call& q = calls[i];
        LH_REQUIRE(q.d && q.x && q.dy && q.grad && q.taps_rs && q.rows <= 1, "lh_wgrad_table_build: bad problem %d", i);
        LH_REQUIRE(q.d->ntaps > 0 && q.d->ntaps <= 64, "lh_wgrad_table_build: ntaps %d out of range (problem %d)", q.d->ntaps, i);
        const long M = (long)q.d->n * q.d->ho * q.d->wo;
        t.stages[i] = (M + base.kps - 1) / base.kps;
        tiles[i] = (long)ceil_div(q.n_out, base.bo) * ceil_div(q.n_in, base.bi) * q.d->ntaps;
        work += t.stages[i] * tiles[i];
        smax = std::max(smax, t.stages[i]);
    }
    t.min_stages = std::max(1, 256 / base.kps);                       // >= 256 pixels per work item
    long L = target_stages;
    if (L <= 0) {
        // split-free when the tiles alone make two rounds of the slots; else the item length that makes about four rounds
        long tsum = 0;
        for (int i = 0; i < n; ++i) tsum += tiles[i];
        L = tsum >= 2 * slots ? smax : std::max(t.min_stages, work / (4 * slots));
    }
    t.L = std::max(L, t.min_stages);
    return LH_OK;
}

// Step 2: every member's split count, its argument block and -- unless the kernel writes the gradient itself -- its slab and fold.
// workspace null (size query): a placeholder slab address, the sizes come out the same.
static int table_members(const lh_wgrad_call* calls, int n, int dtype, void* workspace, TableBuild& t) {
    t.args.resize(n);
    for (int i = 0; i < n; ++i) {
        const lh_wgrad_call& q = calls[i];
        long ns = (t.stages[i] + t.L / 2) / t.L;                      // nearest split count for items of ~L stages
        const long max_split = std::min(128L, std::max(1L, t.stages[i] / t.min_stages));
        ns = std::max(1L, std::min(ns, max_split));
        WgradPlan c = t.base;
        c.sps = (int)((t.stages[i] + ns - 1) / ns);
        c.nsplit = (int)((t.stages[i] + c.sps - 1) / c.sps);
        const size_t per = (size_t)q.n_out * q.n_in;
        // one split, one tap, the gradient dense in [o][i]: the kernel's 16-byte stores ARE the gradient -- no slab, no fold
        const bool direct = c.nsplit == 1 && q.d->ntaps == 1 && !q.accumulate && q.so == q.n_in && q.si == 1 &&
                            ((uintptr_t)q.grad & 15) == 0;
        float* slab = direct ? q.grad : (workspace ? (float*)((char*)workspace + t.ws) : (float*)(uintptr_t)256);
        LH_REQUIRE(wgrad_ring_ok(q.d, 2), "lh_wgrad_table: problem %d does not run on the LDS-DMA weight-gradient kernel", i);
        int rc = wgrad_fill_args(q.d, q.x, q.dy, q.dy_pix_stride, q.n_out, q.n_in, slab, dtype, 0, c, &t.args[i]);
        if (rc) return rc;
        if (direct) continue;
        WreduceArgs ra;
        rc = reduce_prepare(q.d, slab, q.grad, q.n_out, q.n_in, q.so, q.si, q.sr, q.ss, q.taps_rs, q.accumulate, c.nsplit, &ra);
        if (rc) return rc;
        t.fold_lds = std::max(t.fold_lds, wgrad_reduce_lds(ra));
        t.folds.push_back(ra);
        t.ws += up256((size_t)c.nsplit * q.d->ntaps * per * sizeof(float));
    }
    return LH_OK;
}

// Step 3: work-item order.  Workgroup ids are dealt round-robin over the 8 XCDs (block b runs on XCD b % 8, each with a private L2), and the
// items that share operand rows are the taps x tiles of ONE pixel split of ONE layer (every tap of a 3x3 walks the same x / dy rows,
// the channel tiles of a 1x1 share one of the two operands): such a GROUP is laid out on ONE XCD -- consecutive positions of that
// XCD's sub-sequence b = 8 k + x -- so that its members run side by side and read their rows from that L2 once instead of once per
// item from the fabric (PMC, R50's 32-layer table: 3.2 GB of L2 misses per launch for ~1 GB of operands with the per-layer order).
// Groups (at most 16 items) are taken longest item first and handed to the XCD with the least work so far, so every XCD's queue
// runs from long to short items and the queues are equal in cost; queues that hold fewer items end in empty items, which exit at once.
// LH_WGRAD_TABLE_XCD=0: the plain longest-first order with the per-layer XCD remap.
static void table_item_order(int n, TableBuild& t) {
    std::vector<WgradArgs>& args = t.args;
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return args[x].steps_per_split > args[y].steps_per_split; });
    const char* xsw = getenv("LH_WGRAD_TABLE_XCD");
    if (xsw && atoi(xsw) == 0) {
        for (int k = 0; k < n; ++k) {
            const int i = order[k], cnt = args[i].tiles * args[i].ntaps * args[i].nsplit;
            for (int b = 0; b < cnt; ++b) t.items.push_back(int2{i, b});
        }
        return;
    }
    struct Group { int prob, first, count; };                         // `count` consecutive block indices of problem `prob` from `first`
    std::vector<Group> groups;
    // groups of at most 16 items (half an XCD's CUs for the 8-wave tile): the taps x tiles of one split, cut where there are more
    for (int k = 0; k < n; ++k) {
        const int i = order[k], per = args[i].tiles * args[i].ntaps;
        args[i].xcd = 0;                                              // the table places the items; the body must not remap them
        const int parts = (per + 15) / 16, sz = (per + parts - 1) / parts;
        for (int sp = 0; sp < args[i].nsplit; ++sp)
            for (int o = 0; o < per; o += sz) groups.push_back({i, sp * per + o, std::min(sz, per - o)});
    }
    std::stable_sort(groups.begin(), groups.end(), [&](const Group& a, const Group& b) {
        return args[a.prob].steps_per_split > args[b.prob].steps_per_split;
    });
    // longest items first, each group to the XCD with the least work so far: every XCD's queue runs long -> short, equal in cost
    std::vector<int2> queue[8];
    long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const Group& g : groups) {
        int x = 0;
        for (int y = 1; y < 8; ++y)
            if (load[y] < load[x]) x = y;
        for (int b = 0; b < g.count; ++b) queue[x].push_back(int2{g.prob, g.first + b});
        load[x] += (long)g.count * args[g.prob].steps_per_split;
    }
    size_t len = 0;
    for (int x = 0; x < 8; ++x) len = std::max(len, queue[x].size());
    for (size_t pos = 0; pos < len; ++pos)
        for (int x = 0; x < 8; ++x) t.items.push_back(pos < queue[x].size() ? queue[x][pos] : int2{-1, 0});
    while (!t.items.empty() && t.items.back().x < 0) t.items.pop_back();
}

// Step 4: every (problem, block) exactly once, whatever the order: a block left out would leave its slab slice unwritten.
static int table_check_coverage(int n, const TableBuild& t) {
    std::vector<long> first_of(n + 1, 0);
    for (int i = 0; i < n; ++i) first_of[i + 1] = first_of[i] + (long)t.args[i].tiles * t.args[i].ntaps * t.args[i].nsplit;
    std::vector<unsigned char> seen((size_t)first_of[n], 0);
    long placed = 0;
    for (const int2& it : t.items) {
        if (it.x < 0) continue;
        const long cnt = first_of[it.x + 1] - first_of[it.x];
        LH_REQUIRE(it.x < n && it.y >= 0 && it.y < cnt && !seen[(size_t)(first_of[it.x] + it.y)], "lh_wgrad_table_build: internal error in the work-item order");
        seen[(size_t)(first_of[it.x] + it.y)] = 1;
        ++placed;
    }
    LH_REQUIRE(placed == first_of[n], "lh_wgrad_table_build: internal error: %ld of %ld work items placed", placed, first_of[n]);
    return LH_OK;
}

// Step 5: blob layout [WgradArgs x n][int2 items][WreduceArgs x nfold][int2 fold items] into *info and, unless this is the size query
// (host_blob null), the blob itself: only now the argument blocks get the device's zero page.
static int table_emit(int n, TableBuild& t, void* workspace, void* host_blob, size_t host_bytes, lh_wgrad_table_info* info) {
    long n_items = (long)t.items.size(), n_fold_items = 0;
    for (const WreduceArgs& r : t.folds) n_fold_items += wgrad_reduce_blocks(r);
    LH_REQUIRE(n_items < (1L << 30) && n_fold_items < (1L << 30), "lh_wgrad_table_build: too many work items");
    lh_wgrad_table_info o;
    memset(&o, 0, sizeof(o));
    o.bo = t.base.bo; o.bi = t.base.bi; o.kps = t.base.kps; o.depth = t.base.depth;
    o.n_problems = n; o.n_fold = (int)t.folds.size();
    o.n_items = (int)n_items; o.n_fold_items = (int)n_fold_items; o.fold_lds = t.fold_lds;
    o.target_stages = (int)t.L;
    o.off_items = up256(sizeof(WgradArgs) * n);
    o.off_fold_args = o.off_items + up256(sizeof(int2) * n_items);
    o.off_fold_items = o.off_fold_args + up256(sizeof(WreduceArgs) * t.folds.size());
    o.table_bytes = o.off_fold_items + up256(sizeof(int2) * n_fold_items);
    o.workspace_bytes = std::max(t.ws, (size_t)256);
    for (int i = 0; i < n; ++i) o.nsplit_max = std::max(o.nsplit_max, t.args[i].nsplit);
    *info = o;
    if (!host_blob) return LH_OK;                                   // size query
    LH_REQUIRE(workspace && host_bytes >= o.table_bytes, "lh_wgrad_table_build: blob of %zu bytes needs %zu (and a workspace)", host_bytes, o.table_bytes);
    const unsigned char* zero = wgrad_zero_page();
    LH_REQUIRE(zero, "lh_wgrad: cannot resolve the zero page on this device");
    for (WgradArgs& a : t.args) a.zero = zero;
    char* blob = (char*)host_blob;
    memset(blob, 0, o.table_bytes);
    memcpy(blob, t.args.data(), sizeof(WgradArgs) * n);
    memcpy(blob + o.off_items, t.items.data(), sizeof(int2) * t.items.size());
    if (!t.folds.empty()) memcpy(blob + o.off_fold_args, t.folds.data(), sizeof(WreduceArgs) * t.folds.size());
    int2* fi = (int2*)(blob + o.off_fold_items);
    for (int k = 0; k < (int)t.folds.size(); ++k)
        for (int b = 0, cnt = wgrad_reduce_blocks(t.folds[k]); b < cnt; ++b) *fi++ = int2{k, b};
    return LH_OK;
}

extern "C" int lh_wgrad_table_build(const lh_wgrad_call* calls, int n, int dtype, const int* cfg4, int target_stages, void* workspace,
                                    void* host_blob, size_t host_bytes, lh_wgrad_table_info* info) {
    LH_REQUIRE(calls && n >= 1 && cfg4 && info, "lh_wgrad_table_build: bad arguments");
    LH_REQUIRE(lh_dtype_size(dtype) == 2, "lh_wgrad_table_build: 16-bit types only");
    TableBuild t;
    t.base = {cfg4[0], cfg4[1], cfg4[2], cfg4[3], 1, 0};
    if (!wgrad_cfg_compiled(t.base.bo, t.base.bi, t.base.kps, t.base.depth)) {
        lh_set_error("lh_wgrad_table_build: tile %dx%d stage %d depth %d is not compiled in", t.base.bo, t.base.bi, t.base.kps, t.base.depth);
        return LH_ERR_UNSUPPORTED;
    }
    int rc = table_item_length(calls, n, target_stages, t);
    if (!rc) rc = table_members(calls, n, dtype, workspace, t);
    if (rc) return rc;
    table_item_order(n, t);
    rc = table_check_coverage(n, t);
    return rc ? rc : table_emit(n, t, workspace, host_blob, host_bytes, info);
}

extern "C" int lh_wgrad_table_run(const void* table, const lh_wgrad_table_info* info, int dtype, void* stream) {
    LH_REQUIRE(table && info && info->n_items > 0, "lh_wgrad_table_run: bad arguments");
    LH_REQUIRE(dtype == LH_BF16 || dtype == LH_F16, "lh_wgrad_table_run: 16-bit types only");
    hipStream_t s = (hipStream_t)stream;
    const char* blob = (const char*)table;
    const WgradArgs* tab = (const WgradArgs*)blob;
    const int2* items = (const int2*)(blob + info->off_items);
    int rc = LH_OK;
    if (info->run_parts != 2)
        rc = dtype == LH_BF16 ? lh_wgrad_ring_table_launch_bf16(tab, items, info->n_items, info->bo, info->bi, info->kps, info->depth, s)
                              : lh_wgrad_ring_table_launch_f16(tab, items, info->n_items, info->bo, info->bi, info->kps, info->depth, s);
    if (rc == 1) {
        lh_set_error("lh_wgrad_table_run: no kernel for tile %dx%d stage %d depth %d", info->bo, info->bi, info->kps, info->depth);
        return LH_ERR_UNSUPPORTED;
    }
    if (rc) return rc;
    if (info->n_fold_items > 0 && info->run_parts != 1) {
        hipLaunchKernelGGL(wgrad_reduce_table_kernel, dim3(info->n_fold_items), dim3(256), info->fold_lds, s,
                           (const WreduceArgs*)(blob + info->off_fold_args), (const int2*)(blob + info->off_fold_items));
        LH_LAUNCH_CHECK("wgrad_reduce_table launch");
    }
    return LH_OK;
}
