// K10's tile -> workgroup mappings (included by blend_forward.hip, and by blend_features.hip for the columns mapping): the six that were built and measured, selected at run time by
// BlendArgs::row_group, and the history of their measurements. The product library always passes kColumnsTopDown (api.hip); the dev library passes what
// fgs_debug_set_option(10, ..) set. The product kernels still compile all six arms: with the columns arm alone they are 240 instructions shorter each,
// but the allocator then puts two more moves and a wait into the walk's trip of blend_kernel<true>, and K10 measured 1 - 2 % slower in 14 of 14
// alternating pairs (profiles/k10_exhibits_split.txt, section 6). The comments stand as they were written in blend_forward.hip.
#pragma once
#include "fgs_kernels.h"

namespace fgs {

// Which tile does workgroup `block` blend? The hardware deals workgroups to the 8 XCDs round-robin (XCD = block % 8), and a Gaussian's
// records are re-read by every tile it overlaps -- from the XCD's own L2 if the neighbouring tiles run there. Round 1 gave every XCD one
// contiguous band of tile rows. A per-tile timeline (tools/k10_timeline.sh, profiles/archive/r02_k10_timeline_before.txt) showed what that costs: the
// top band of the image is nearly empty (XCD 0 had 30 ms of summed tile time against 44-47 ms for the others at S2, 47 against 210-220 ms on the
// layered scene, and idled for a third / two thirds of the kernel), and the heaviest rows -- the bottom of the image, nearest to the camera --
// came LAST in every band. Alternative mapping (row_group >= 1): groups of `row_group` consecutive tile rows are dealt to the XCDs in turn over
// the whole image and every XCD walks its rows from the bottom of the image upwards (heaviest first). Measured (tools/ab_tile_rows.py,
// profiles/archive/r02_ab_tile_rows.txt; training / inference blend): S2 bands 0.163 / 0.157 ms, g = 1 0.177 / 0.171, g = 2 0.189 / 0.182 -- at two
// blended buckets per tile the kernel lives on the L2 locality of vertical neighbours; layered scene (11 buckets per tile) bands 0.725 / 0.700,
// g = 1 0.663 / 0.646, g = 2 0.654 / 0.633 -- there balance wins 10 %. Bands walked bottom-up (255): no difference. Which of the two a scene
// wants depends on how deep its tiles blend, which the host does not know at launch: the DEFAULT stays the bands (the benchmark workload),
// fgs_debug_set_option(10, g) selects the other. Returns n_tiles for padding workgroups.
// Round 3, measured on one box (tools/ab_tile_plan.py, profiles/archive/r03_ab_tile_plan.txt; training blend S2 / layered scene, ms):
//   bands (round 1/2 default)                          0.168 / 0.765
//   single rows interleaved                            0.179 / 0.657
//   8 x 10 blocks weighed on the device by their bucket counts, sorted, dealt heaviest-first to the least-loaded XCD
//   (row_group == kPlannedBlocks, plan_tiles_kernel)   0.181 / 0.646   -- balance, but the scattered block order costs S2 what rows cost
//   the same blocks in natural order, XCD x = block column x          0.164 / 0.673
//   COLUMNS (kColumnsTopDown, the default now): XCD x owns the vertical strip of tile columns [x w, (x + 1) w), w = ceil(grid_w / 8),
//   and walks it row by row from the top                              0.164 / 0.669   (bottom-up: 0.177 / 0.695)
// The work gradient of a rendered view is vertical (sky on top, near ground at the bottom), so a vertical strip per XCD is balanced by
// construction and as compact as a band: -2 % at S2 and -12 % on the layered scene against the bands, closed form, no device data. The
// device-side plan stays as an A/B option (it wins 3 % more on the layered scene and loses 10 % at S2).
constexpr unsigned kBandsBottomFirst = 255u;     // row_group value: the round-1 bands, each walked from its last tile to its first
__device__ __forceinline__ unsigned tile_of_workgroup(const unsigned block, const unsigned grid_w, const unsigned n_tiles, const unsigned row_group,
                                                      const uint32_t* __restrict__ plan = nullptr, const unsigned grid_h = 0u) {
    if (row_group == kPlannedBlocks) {
        const unsigned bw = (grid_w + kPlanBlocksX - 1) / kPlanBlocksX, bh = (grid_h + kPlanBlocksY - 1) / kPlanBlocksY;   // = plan[0], plan[1]
        const unsigned per_block = bw * bh;
        const unsigned xcd = block % kXcds, q = block / kXcds;
        const unsigned slot = q / per_block, local = q - slot * per_block;
        if (slot >= kPlanBlocksPerXcd) return n_tiles;
        const unsigned b = plan[kPlanHeader + xcd * kPlanBlocksPerXcd + slot];                 // wave-uniform: a scalar load
        const unsigned ly = local / bw, lx = local - ly * bw;
        const unsigned tx = (b % kPlanBlocksX) * bw + lx, ty = (b / kPlanBlocksX) * bh + ly;
        return (tx < grid_w && ty < grid_h) ? ty * grid_w + tx : n_tiles;
    }
    if (row_group == kColumnsTopDown || row_group == kColumnsBottomUp) {
        // every XCD owns one vertical strip of the image, ceil(grid_w / 8) tiles wide, and walks it row by row: compact (the strip's rows
        // follow each other in time, so a Gaussian's record is still in this XCD's L2 when the row below needs it), and balanced by
        // construction against the dominant work gradient of a rendered scene -- the vertical one (sky / far background on top, near
        // ground at the bottom): every XCD gets every image row
        const unsigned bw = (grid_w + kXcds - 1) / kXcds;
        const unsigned xcd = block % kXcds, q = block / kXcds;
        const unsigned r = q / bw, c = q - r * bw;
        const unsigned tx = xcd * bw + c, ty = row_group == kColumnsTopDown ? r : grid_h - 1u - r;
        return (tx < grid_w && r < grid_h) ? ty * grid_w + tx : n_tiles;
    }
    if (row_group == kBandsThroughPlan) {                                                   // A/B: what does the plan's load alone cost?
        const unsigned per_xcd = (n_tiles + kXcds - 1) / kXcds;
        const unsigned tile = (block % kXcds) * per_xcd + block / kXcds + (plan[kPlanHeader + (block % kXcds) * kPlanBlocksPerXcd] >> 30);
        return tile < n_tiles ? tile : n_tiles;
    }
    if (row_group == 0u || row_group == kBandsBottomFirst) {                                // one contiguous band per XCD, top-down or bottom-up
        const unsigned per_xcd = (n_tiles + kXcds - 1) / kXcds;
        const unsigned idx = block / kXcds;
        const unsigned tile = (block % kXcds) * per_xcd + (row_group == 0u ? idx : per_xcd - 1u - idx);
        return tile < n_tiles ? tile : n_tiles;
    }
    const unsigned n_rows = n_tiles / grid_w;
    const unsigned xcd = block % kXcds, j = block / kXcds;
    const unsigned k = j / grid_w, col = j - k * grid_w;                                   // k-th row this XCD walks
    const unsigned cycles = (n_rows + kXcds * row_group - 1) / (kXcds * row_group);        // groups per XCD
    if (k >= cycles * row_group) return n_tiles;
    const unsigned kk = cycles * row_group - 1u - k;                                       // bottom of the image first
    const unsigned row = (kk / row_group) * (kXcds * row_group) + xcd * row_group + kk % row_group;
    return row < n_rows ? row * grid_w + col : n_tiles;
}
// Round 5 tried the strips as per-XCD QUEUES with stealing (a workgroup pops the next tile of the strip of the XCD it runs on, hardware XCC_ID, and takes
// from the fullest other strip once its own is empty) for object-centric scenes, whose outer strips are nearly empty (bench.py's surface scene: 5.8 ms of
// summed tile time on XCD 0 against 108 ms on XCD 3). Measured (tools/ab_k10_mapping.py at the commit that had it): the one returning atomic per workgroup
// costs S2 0.145 -> 0.176 ms (10 800 pops onto eight words), a device-scope snapshot of the queue heads in front of it 0.73 ms; and the scene that
// motivated it gains nothing from balance alone -- the device-side block plan, which balances it, measures 0.366 against 0.387 ms -- because its span is
// the serial walk of single tiles with lists of thousands (389 us for one tile of 3 860 walked entries). Removed.
// the launch grid of a mapping: its tiles and its padding workgroups. A mapping that reads the plan is launched with one (api.hip: bucket_scan_and_mapping).
static unsigned columns_grid(const unsigned grid_w, const unsigned grid_h) { return kXcds * ((grid_w + kXcds - 1) / kXcds) * grid_h; }   // kColumnsTopDown / kColumnsBottomUp
static unsigned blend_grid(const BlendArgs& a) {
    if (a.row_group == kColumnsTopDown || a.row_group == kColumnsBottomUp) return columns_grid(a.grid_w, a.grid_h);
    if (a.row_group == kBandsThroughPlan) return ((a.n_tiles + kXcds - 1) / kXcds) * kXcds;
    if (a.row_group == kPlannedBlocks)
        return kPlanBlocks * ((a.grid_w + kPlanBlocksX - 1) / kPlanBlocksX) * ((a.grid_h + kPlanBlocksY - 1) / kPlanBlocksY);
    if (a.row_group == 0u || a.row_group == kBandsBottomFirst) return ((a.n_tiles + kXcds - 1) / kXcds) * kXcds;
    const unsigned grid_h = a.n_tiles / a.grid_w;
    const unsigned cycles = (grid_h + kXcds * a.row_group - 1) / (kXcds * a.row_group);
    return kXcds * cycles * a.row_group * a.grid_w;
}

}  // namespace fgs
