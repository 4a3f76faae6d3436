// The int8 GEMM's plan (host only: no kernel lives in this file): plan_gemm holds the selection ladder of DESIGN.md §4 once; launch_gemm
// executes its plan, describe_gemm_plan prints it, and every "would launch_gemm take ...?" question of the API layer is a question to it.
#include "mixq_launch.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace mixq {

constexpr int KSLICE = 128;  // bytes of K per LDS row (int8 elements)

// ---- K split over workgroups for the two small-tile forms with in-workgroup split (see the kernel header) ------------
static std::atomic<int> g_xsplit_force{-1}; // -1 automatic, 0 off, 2 / 4 / 8 / 16 forced where the shape allows it
static std::atomic<int> g_xsplit_max_bm{64}; // tallest tile the plan may take (knob 63 / 65: 32 / 64 rows)

// 0 = not used.  Applies to the problems launch_epi gives to the 32x64 / 64x64 tiles with 4 K groups (at most 256 tiles):
// XS = 4 / 2 more workgroups per tile while that still leaves at most one workgroup per CU, and K is long enough for
// each of the 4 x XS parts to keep a few slices.
// The plan: which of the two tilings, and how many workgroups per tile.  The tiling is the first of 32x64 / 64x64 that
// gives at most 128 tiles (so that at least two workgroups per tile fit on the chip at one workgroup per CU).
struct XSplitPlan {
    int xs;    // 0 = not used
    int bm;    // tile rows: 32 or 64 (tile columns: 64)
    int tiles;
};
static XSplitPlan xsplit_plan(int M, int N, int K)
{
    XSplitPlan none{0, 0, 0};
    const int force = g_xsplit_force.load();
    if (force == 0 || M <= 4) return none;
    if (force < 0 && M <= 16 && K < 16384) return none; // M <= 16: the skinny kernel unless K is very long (measured)
    const int64_t n64 = (N + 63) / 64;
    const int nk = (K + KSLICE - 1) / KSLICE;
    if (force < 0 && nk < 64) return none; // automatic: K >= 8192 (measured: at K = 4096 the exchange eats the gain)
    // per tiling: as many workgroups per tile as leave at most one workgroup per CU and 16 slices per workgroup (forced
    // factors: 8 slices); the tiling that puts more workgroups on the chip wins, 64x64 on a tie (measured: equal or up to
    // 26 % faster than 32x64 -- fewer operand bytes per MAC; a 128x64 tiling with 2 K groups was measured too: slower)
    auto factor = [&](int64_t tiles) {
        if (tiles > 128) return 0;
        if (force > 0) return ((int64_t)force * tiles <= 256 && nk >= 8 * force) ? force : 0;
        int xs = 16;
        while (xs > 1 && ((int64_t)xs * tiles > 256 || nk < 16 * xs)) xs >>= 1;
        return xs >= 2 ? xs : 0;
    };
    const int max_bm = g_xsplit_max_bm.load();
    XSplitPlan best = none;
    for (int bm = 32; bm <= max_bm; bm *= 2) {
        if (bm > 32 && M <= bm / 2) break; // a taller tile would only add empty rows
        const int64_t tiles = (int64_t)((M + bm - 1) / bm) * n64;
        const int xs = factor(tiles);
        if (xs != 0 && tiles * xs >= (int64_t)best.tiles * best.xs) best = XSplitPlan{xs, bm, (int)tiles};
    }
    return best;
}

size_t gemm_xsplit_workspace_size(int M, int N, int K)
{
    const XSplitPlan pl = xsplit_plan(M, N, K);
    if (pl.xs == 0) return 0;
    return kSplitkWordsBytes + (size_t)pl.tiles * pl.xs * (size_t)(pl.bm * 64 * 4);
}

size_t gemm_xsplit_workspace_bound() { return kSplitkWordsBytes + (size_t)256 * 64 * 64 * 4; } // <= 256 workgroups x 16 KiB

// ---- mid-M "deep" form (round 5): 128 x 128 tiles, 4 LDS stages really in flight (ADMA), K split over XS workgroups per tile ----
// 129..512 rows are the band furthest below either roofline: the 256 x 256 / 128 x 256 ping-pong tiles cover a
// quarter to a half of the CUs there, and the small two-barrier tiles run their slices one memory round trip at a time.  This form
// puts (about) one workgroup of a 128 x 128 tile on every CU -- the tiles alone where there are enough of them, 2 / 4 / 8 workgroups
// per tile along K otherwise -- and keeps three slices in flight behind the one being multiplied.  Same int32 sums, same epilogue.
static std::atomic<int> g_deep_late{1}; // measurement knob 1238 (default) / 1239: the second half of the waves issue their copies after / before their MFMAs
static std::atomic<int> g_deep_force{-1}; // -1 automatic, 0 off, 1 / 2 / 4 / 8: forced workgroups per tile (knobs 1240 / 1241 + xs); + 10: the 8-wave build
struct DeepPlan {
    int xs;    // 0 = not used; workgroups per 128 x 128 tile otherwise
    int tiles;
    int waves8; // build: 0 = 4 waves x 64 x 64, 1 = 8 waves x 64 x 32 (4 stages), 2 = 8 waves, 5 stages, 3 = round 6: copy-only waves + one barrier per pair of slices (gemm_mid_kernels.hip)
};
// The automatic rule: a table over (128 x 128 tiles, K slices), read off a sweep of every build x split against the selection as it
// was, on COLD weights (a model's layer never finds its weights cache-resident), profiles/r05_deep_form_sweep_cold.txt -- 110 cells
// over the ten (N, K) of BASELINE.json's configs, 80..1024 rows.  The form wins 8..35 % exactly where it puts 140..256 workgroups
// on the chip and the alternatives leave CUs idle or take their slices one round trip at a time:
//   tiles 140..256, K 3072..5120        -> the tiles alone            (12288 x 4096 at 129..256 rows: 35.0 -> 28.3 us)  [and > 512 tiles of 64 x 64]
//   tiles  70..128, K 5120..12800       -> 2 workgroups per tile      (4096 x 11008 at 320..512 rows: 42.8 -> 36.1 us)
//   tiles  36..64,  K 8192..20480       -> 4                          (4096 x 11008 at 129..256 rows: 35.4 -> 30.9 us)
//   tiles  20..32,  K >= 25600          -> 8                          (1024 x 28672 at 257..512 rows: 46.1 -> 34.1 us)
// Everywhere else it is level or behind (the ping-pong tiles multiply a slice in less than half the time per CU; warm weights:
// level) and is not used.  8 waves x (64 x 32) beat 4 waves x (64 x 64) in every cell; a fifth LDS stage changed nothing, neither did
// 16 waves x (32 x 32); the same loop on 128 x 256 tiles is behind the ping-pong kernel of that tile (profiles/r05_deep_form_builds.txt).
static std::atomic<int> g_deep_mid{1}; // measurement knob 1420 (default) / 1421: the automatic plan takes the round-6 schedule from 129 rows on / never
static DeepPlan deep_plan_auto(int M, int N, int K, int tiles, int nk)
{
    (void)N;
    const int cus = num_cus();
    if (cus != 256) return DeepPlan{0, 0, 0}; // (the table counts workgroups against the 256 CUs it was measured on)
    // (first row: only where the 64 x 64 tiles are past their forms with K split inside the workgroup -- more than 512 of them;
    //  below that those are ahead: 448 x 4608 x 3584 19.5 vs 23.7 us, 288 x 6144 x 4096 21.6 vs 26.0, validation sweep of the table)
    const int64_t wg64 = (int64_t)((M + 63) / 64) * ((N + 63) / 64);
    // (round 6) from 129 rows on every row of the table runs the round-6 schedule of the same tiles (gemm_mid_kernels.hip; whole 128-byte slices only):
    // cold, all ten BASELINE (N, K), 35 cells: ahead of the round-5 build in 33, by 6-25 % (12288 / 11008 x 4096 at 160..256 rows 27-28 -> 24.4-26.2 us,
    // 3584 x 8192 at 320 / 384 rows 30.5 -> 26 us, 4608 x 3584 at 512 rows 24.7 -> 20.6, 1280 x 8192 at 1024 rows 30.4 -> 24.3, 1024 x 28672 at 320 rows
    // 34.7 -> 31.3); level at 97..128 rows, which keep the round-5 build (profiles/r06_mid_final_sweep_cold.txt)
    const int mid = M > 128 && K % KSLICE == 0 && g_deep_mid.load() ? 3 : 1;
    if (tiles >= 140 && tiles <= 256 && nk >= 24 && nk <= 40 && wg64 > 512) return DeepPlan{1, tiles, mid}; // (measured at K = 3584 .. 5120 only)
    // (97..128 rows on one row of 70..128 tiles at K = 3072..5120: two workgroups per tile put 140..256 workgroups on the chip where the
    //  64 x 64 tiles with two K groups inside the workgroup run 1.5 rounds -- profiles/r05_int8_forms_cold.jsonl: 12288 x 4096 at 128 rows
    //  24.2 -> 22.7 us, 11008 x 4096 24.2 -> 22.0; at 96 rows -1..-5 %, at 72 rows level: from 97 rows)
    if (M > 96 && M <= 128 && tiles >= 70 && tiles <= 128 && nk >= 24 && nk <= 40) return DeepPlan{2, tiles, 1};
    if (M <= 128) return DeepPlan{0, 0, 0};
    // (second row at K < 8192 only past 256 tiles of 64 x 64: one workgroup per CU of those with K split four ways inside it is
    //  ahead below -- 160 / 192 x 5120 x 5120: 20.0 / 20.9 vs 23.1 / 23.5 us, profiles/r05_int8_forms_cold.jsonl)
    if (tiles >= 70 && tiles <= 128 && nk >= 40 && nk <= 100 && (nk >= 64 || wg64 > 256)) return DeepPlan{2, tiles, mid};
    if (tiles >= 36 && tiles <= 64 && nk >= 64 && nk <= 160) return DeepPlan{4, tiles, mid};
    if (M > 256 && tiles >= 20 && tiles <= 32 && nk >= 200) return DeepPlan{8, tiles, mid};
    return DeepPlan{0, 0, 0};
}
static DeepPlan deep_plan(int M, int N, int K)
{
    DeepPlan none{0, 0, 0};
    const int force = g_deep_force.load();
    if (force == 0 || M <= 64) return none;
    const int64_t tiles = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
    const int nk = (K + KSLICE - 1) / KSLICE;
    if (tiles > 4096) return none;
    if (force > 0) {
        const int xs = force % 10;
        if (xs > 1 && tiles * xs > 768) return none; // (the parked tiles must fit the scratch bound: 64 KiB per workgroup)
        return (xs == 1 || xs == 2 || xs == 4 || xs == 8) && nk >= 4 * xs ? DeepPlan{xs, (int)tiles, force / 10} : none;
    }
    return deep_plan_auto(M, N, K, (int)tiles, nk);
}
size_t gemm_deep_workspace_size(int M, int N, int K)
{
    const DeepPlan pl = deep_plan(M, N, K);
    if (pl.xs <= 1) return 0;
    // a parked tile is 128 x 128 or -- the mid kernel's 96-wide tiles, gemm_mid_tile_width -- 128 x 96 int32: room for whichever count x size is larger
    const size_t t96 = (size_t)((M + 127) / 128) * ((N + 95) / 96);
    const size_t b128 = (size_t)pl.tiles * (128 * 128 * 4), b96 = t96 * (128 * 96 * 4);
    return kSplitkWordsBytes + (b128 > b96 ? b128 : b96) * pl.xs;
}

static std::atomic<int> g_force_cfg{-1}; // measurement knob (variant 10 + i): force tile configuration i
static std::atomic<int> g_skinny_kw{0}; // measurement knob: force the K-split width (0 = auto)

// Schedule selection.  0 = auto (ping-pong 256x256 kernel when the problem fills the chip with 256x256 tiles, else the
// 2-barrier kernel in a smaller tile), 1 = always the 2-barrier kernel, 2 = ping-pong whenever M > 4.
// (The persistent ping-pong experiment of round 1 -- measured to lose -- is in the history: tools/experimental/README.md.)
// Set through mixq_debug_set_gemm_variant() (tests, A/B measurements) or MIXQ_GEMM_VARIANT=v1|pp in the environment.
static std::atomic<int> g_variant{-1};
static std::atomic<int> g_skinny_wide{0};
static std::atomic<int> g_qa_frag{1};
bool qa_frag_enabled() { return g_qa_frag.load() != 0; }

void set_gemm_variant(int v)
{
    if (v == 1238 || v == 1239) {
        g_deep_late.store(v == 1238);
        return;
    }
    if (v == 1420 || v == 1421) { // the automatic deep plan: round-6 schedule from 129 rows on (1420, default) / the round-5 build everywhere (1421)
        g_deep_mid.store(v == 1420);
        return;
    }
    if (v >= 1430 && v <= 1433) { // round-6 mid kernel: tile width by rule (1430, default: 96 where that puts more workgroups on the chip) / 128 always (1431)
        set_mid_bn(v - 1430);
        return;
    }
    if (v >= 1410 && v <= 1413) { // round-6 mid kernel: tile rows start at different K slices: 1413 by the measured rule (default: 4..7 tile rows, K not split) / 1411 never / 1410 where K is not split over workgroups / 1412 always
        set_mid_rot(v == 1410 ? 1 : v == 1411 ? 0 : v == 1412 ? 2 : 3);
        return;
    }
    if (v >= 1240 && v <= 1279) { // mid-M deep form: 1240 automatic, 1241 off, 1241 + xs (1242 / 1243 / 1245 / 1249) forced, + 10 the 8-wave build, + 30 the round-6 schedule
        g_deep_force.store(v == 1240 ? -1 : v - 1241);
        return;
    }
    if (v >= 1300 && v <= 1312) { // quantisers: rows up to which one 256-thread block takes one row: 1300 the measured rules (default), 1301 + n: 64 << n rows
        set_quant_block_rows(v == 1300 ? -1 : 64 << (v - 1301));
        return;
    }
    if (v >= 1290 && v <= 1292) { // tile kernels, non-temporal weight copies on a single tile row: 1290 by rule, 1291 never, 1292 always
        set_tile_nt(v - 1290);
        return;
    }
    if (v >= 884 && v <= 887) { // decode-batch GEMM, row-major weights in 256-byte runs through LDS: 884 on, non-temporal from 32 MiB (default), 885 off, 886 / 887 on with non-temporal loads always / never
        set_skinny_wrows(v == 884 ? 1 : v == 885 ? 0 : v == 886 ? 2 : 3);
        return;
    }
    if (v >= 880 && v <= 883) { // registered weight images in the decode-batch GEMM: 880 automatic, 881 plain loads, 882 non-temporal loads, 883 ignored
        set_skinny_wfrag(v - 880);
        return;
    }
    if (v >= 894 && v <= 896) { // fragment-major skinny form: feature tiles per workgroup automatic / 1 / 2
        set_skinny_nt(v - 894);
        return;
    }
    if (v == 892 || v == 893 || v == 897) { // probe: the skinny kernel for every N up to 32 rows (892) / up to 64 rows (897) / the
        g_skinny_wide.store(v == 892 ? 1 : v == 897 ? 2 : 0); // measured rule (893, default)
        return;
    }
    if (v == 890 || v == 891) { // fragment-major qA for mixq_enqueue's decode batches: 890 off (row-major), 891 on (default)
        g_qa_frag.store(v == 891 ? 1 : 0);
        return;
    }
    if (v >= 92 && v <= 99) { // skinny-kernel ablations (measurement only, wrong results): 92 + ABL - 1
        g_skinny_kw.store(21 + (v - 92));
        g_force_cfg.store(-1);
        g_variant.store(0);
        return;
    }
    if (v == 859 || v == 8590) { // fpA_intB skinny form, 16 columns per wave x 8 / 16 waves (measurements, up to 16 tokens)
        set_wo_force(v == 859 ? 309 : 310, -2);
        return;
    }
    if (v >= 856 && v <= 858) { // decode batches (2..4 tokens) through the fpA_intB skinny form: 856 always, 857 never, 858 automatic
        set_wo_force(306 + (v - 856), -2);
        return;
    }
    if (v >= 850 && v <= 855) { // fpA_intB skinny form (5..32 tokens): 850 automatic, 851 off, 852..855 a fixed shape
        set_wo_force(300 + (v - 850), -2);
        return;
    }
    if (v == 848 || v == 849) { // fpA_intB skinny form, non-temporal loads of weights >= 32 MiB: 848 on (default), 849 off
        set_wo_force(v == 848 ? 500 : 501, -2);
        return;
    }
    if (v >= 845 && v <= 847) { // fpA_intB wide form, weights through registers instead of LDS: 845 automatic, 846 never, 847 always
        set_wo_force(400 + (v - 845), -2);
        return;
    }
    if (v == 843 || v == 844) { // second pass of the two-pass form on 256- / 128-row tiles
        set_wo_force(v == 843 ? 203 : 204, -2);
        return;
    }
    if (v >= 840 && v <= 842) { // fpA_intB two-pass form: 840 automatic (from 1280 tokens), 841 never, 842 whenever the shape allows
        set_wo_force(200 + (v - 840), -2);
        return;
    }
    if (v >= 831 && v <= 836) { // fpA_intB wide-form configuration 1..4 (w8a16_gemm_kernels.hip kWoCfg)
        set_wo_force(v - 830, -2);
        return;
    }
    if (v >= 800 && v < 816) { // fpA_intB wide-form ablations (measurement only, wrong results): 800 + ABL
        set_wo_force(100 + (v - 800), -2);
        return;
    }
    if (v >= 80 && v <= 89) { // fpA_intB GEMM (w8a16_gemm_kernels.hip): 80 automatic, 81 narrow passes, 82 / 84 wide form with
                              // 128- / 256-row tiles; 85 K split automatic, 86..89: 1 / 2 / 4 / 8 workgroups per tile
        if (v <= 84) set_wo_force(v == 80 ? -1 : v == 81 ? 0 : v == 82 ? 3 : 4, -2);
        else set_wo_force(-2, v == 85 ? -1 : 1 << (v - 86));
        return;
    }
    if (v == 90 || v == 91) { // 90: split workgroups never wait for their partners (all but the last arriver defer), 91: default
        set_splitk_patience(v == 90 ? 0u : 3000u);
        return;
    }
    if (v >= 70 && v <= 79) { // K split over workgroups (ping-pong kernel): 70 off, 72 / 74 / 78 forced factor, 79 automatic
        set_splitk_force(v == 79 ? -1 : v - 70);
        if (v == 70 || v == 79) g_xsplit_force.store(v == 79 ? -1 : 0);
        return;
    }
    if (v >= 60 && v <= 69) { // the same for the small-tile kernels: 60 off, 62 / 64 / 68 / 66 forced 2 / 4 / 8 / 16, 69 auto
        if (v == 63 || v == 65) { // (tallest tile of the plan: 32 / 64 rows)
            g_xsplit_max_bm.store(v == 63 ? 32 : 64);
            return;
        }
        g_xsplit_force.store(v == 69 ? -1 : v == 66 ? 16 : v - 60);
        return;
    }
    if (v >= 40 && v < 100) { // 40 + kw: skinny kernel with kw K-split waves (measurements)
        g_skinny_kw.store(v - 40);
        g_force_cfg.store(-1);
        g_variant.store(0);
        return;
    }
    g_skinny_kw.store(0);
    if (v < 0) { // (mixq_debug_reset) forget a forced schedule: MIXQ_GEMM_VARIANT in the environment is read again
        g_force_cfg.store(-1);
        g_variant.store(-1);
        return;
    }
    if (v >= 10 && v < 100) { // 10 + i: the 2-barrier kernel in tile configuration i (measurements)
        g_force_cfg.store(v - 10);
        g_variant.store(1);
        return;
    }
    g_force_cfg.store(-1);
    g_variant.store(v);
}

static int gemm_variant()
{
    int v = g_variant.load();
    if (v < 0) {
        const char* e = getenv("MIXQ_GEMM_VARIANT");
        v = (e && e[0] == 'v' && e[1] == '1') ? 1 : (e && e[0] == 'p' && e[1] == 'p') ? 2 : 0;
        g_variant.store(v);
    }
    return v;
}

// 128 x 256 ping-pong tiles (gemm_pp128_kernels.hip) win where they fill most of ONE wave of the chip and K is short enough
// that the 256 x 256 form's K split over workgroups would not amortise its exchange: measured on 90 mid-size shapes
// (tools/pp128_sweep.sh, profiles/r02_pp128_sweep.txt): 88..256 tiles at K < 8192 (-3..-21 %), 160..256 tiles at
// 8192 <= K < 10240 (-4..-5 %); more than one wave of tiles, fewer than ~88 tiles or longer K: the other forms.
bool gemm_pp128_wins(int M, int N, int K)
{
    if (M <= 128) return false;
    const int64_t tm = (M + 127) / 128, t = tm * ((N + 255) / 256);
    const int nk = (K + 127) / 128, cus = num_cus();
    if (t > cus) return false;
    // tiles weighted by the share of their rows that exist (round 4, tools/midm_cfg_sweep.py in steady state: 192 x 12288 x 4096 = 96
    // tiles three quarters full ran 26.2 us here against 23.8 us on plain 64 x 64 tiles; every other mid-M cell within 2 % of its best)
    const int64_t t_rows = tm <= 2 ? t * M : t * 128, full = tm <= 2 ? tm * 128 : 128; // (measured for one / two tile rows only)
    if (nk < 64) return 256 * t_rows >= (int64_t)88 * cus * full;
    if (nk < 80) return 256 * t_rows >= (int64_t)160 * cus * full;
    return false;
}

static std::atomic<const char*> g_last_kernel{"none"}; // reporting only (bench.py's roofline.kernel)
const char* last_gemm_kernel() { return g_last_kernel.load(std::memory_order_relaxed); }
void note_gemm_kernel(const char* name) { g_last_kernel.store(name, std::memory_order_relaxed); }

// The decode-batch rule: the weight-streaming skinny kernel takes this call (variant: the schedule knob, read once by plan_gemm)
static bool takes_skinny(const GemmParams& p, int epi, int variant)
{
    const bool frag = p.a_frag == 1; // the caller holds (or, probing, could produce) the fragment-major qA image
    // long K: the small tiles with K split over workgroups -- unless the image is there, N / 16 workgroups fill the chip and K is
    // not longer than 12288 (operator us, K split vs skinny on the image: 4096 x 11008 at 32 / 48 rows 20.9 / 21.4 vs 17.6 / 20.0,
    // 8192 x 8192 at 32 22.4 vs 19.9; 3584 x 18944 25.6 vs 36.9 and 1024 x 28672 24.2 vs 50.0 stay with the K split)
    // (round 4, re-fitted on COLD weights -- a model's decode step never finds a layer's weights cache-resident --
    //  profiles/r04_decode_batch_longk_probe.txt, operator us, small-tile K split vs skinny on the qA image, 32 rows: 1280 x 8192 16.8 / 15.1,
    //  2048 x 8192 17.0 / 15.1, 3584 x 8192 18.6 / 16.2, 1024 x 8192 16.3 / 14.4; beyond K = 8192 the K split stays (5120 x 13824 32.9 /
    //  35.0, 8192 x 16384 41.2 / 47.5, 3584 x 18944 29.8 / 39.7, 1024 x 28672 27.9 / 52.1) -- UNLESS the weight has a registered image
    //  (gemm_skinny_kernels.hip), which the skinny kernel streams 15-20 % faster: 5120 x 13824 27.8, 8192 x 16384 37.2, 4096 x 16384 29.2
    //  -> 24.1, 2560 x 12288 21.6 -> 18.2, 512 x 8192 15.8 -> 12.5; at 48 rows 3584 x 8192 19.7 -> 17.0, 1280 x 8192 16.7 -> 16.0.)
    const bool img = frag && p.b_image != nullptr;
    const int c16 = 16 * num_cus();
    const bool skinny_on_image = frag && ((p.N >= c16 && p.K <= 12288) || (p.M <= 32 && p.N >= 1024 && p.K <= 8192) ||
                                          (img && p.M <= 32 && p.N >= 512 && p.K <= 16384) ||
                                          (img && p.M <= 48 && p.N >= 1024 && p.N <= c16 && p.K <= 12288));
    const bool xsplit_wins = epi != EPI_INT32 && p.splitk_ws != nullptr && p.K >= 8192 && xsplit_plan(p.M, p.N, p.K).xs != 0 &&
                             !skinny_on_image;
    // 33..64 rows (fragment-major qA image only), round 4 on COLD weights (profiles/r04_decode_batch_k4096_probe.txt, operator us, tiles vs
    // skinny / skinny on a registered weight image): 12288 x 4096 at 48 rows 22.7 vs 25.1 / 21.7, 11008 x 4096 22.4 / 24.4 / 20.6,
    // 8192 x 4096 19.1 / 18.6 / 16.0, 6144 x 4096 at 64 rows 19.1 / 20.7 / 18.5, 5120 x 5120 (32 features per workgroup) at 48 rows
    // 22.0 / 23.5 / 19.7, at 64 rows 22.2 / 26.0 / 23.0, 4096 x 4096 at 64 rows 17.9 / 14.4 / 13.2.  (Round 3 had fitted this warm:
    // 48 rows up to N = 12288, 64 rows up to 6144 whatever the weight's layout.)
    const bool one_tile = skinny_feature_tiles(p.M, p.N, p.K, false) == 1 || skinny_feature_tiles(p.M, p.N, p.K, true) == 1;
    // (round 5) with the row-major weight read in 256-byte runs (K % 256 == 0: then one_tile holds without an image) the skinny kernel keeps
    // 33..48 rows up to N = 12288 at K <= 5120 (selection check, operator us, tiles vs skinny: 48 x 12288 x 4096 19.2 / 17.4 warm, 22.4 / 21.6 cold)
    const bool runs = p.K % 256 == 0 && p.K <= 5120 && skinny_feature_tiles(p.M, p.N, p.K, false) == 1;
    // (the rule with an image is a SUPERSET of the rule without: a producer that probed without the weight pointer -- mixq_qa_layout --
    //  and wrote the fragment-major image must find the consumer agreeing whatever the registry holds)
    // (two feature tiles per workgroup on the 256-byte-run route, N = 5120..8192, K <= 8192: ahead of the tiles up to 64 rows -- gemm_skinny_kernels.hip)
    const bool runs2 = frag && p.K % 256 == 0 && p.K <= 8192 && skinny_feature_tiles(p.M, p.N, p.K, false) == 2 && p.N >= 5120 && p.N <= 8192;
    // (17..32 rows beyond N = 12288: with two feature tiles per workgroup on the run route the skinny kernel stays ahead of the tiles up to N ~ 20000 at
    //  K <= 5120 -- 18944 x 3584 at 32 rows 25.1 -> 23.0 / 23.6 -> 21.3 us on two boxes)
    const bool wide2 = frag && p.K % 256 == 0 && p.K <= 5120 && p.N > 12288 && p.N <= 20480 && skinny_feature_tiles(p.M, p.N, p.K, false) == 2;
    const bool rows_plain = (p.M <= 48 && p.N <= (runs ? 12288 : 8192) && one_tile) || (p.M <= 64 && p.N <= 4096) || (runs2 && p.M <= 64);
    const bool rows_33_64 = frag && (rows_plain || (img && ((p.M <= 48 && p.N <= 12288) || (p.M <= 64 && p.N <= 6144 && one_tile))));
    const int wide = g_skinny_wide.load();
    return variant != 1 && !xsplit_wins && gemm_skinny_supported(p) &&
           (p.M <= 16 || (p.M <= 32 && (p.N <= 12288 || wide2 || wide != 0)) || rows_33_64 || (p.M <= 64 && wide == 2));
    // (33..64 rows, fragment-major image only, operator us, tiles vs skinny: 4096 x 4096 at 40 / 48 / 64 rows 13.4 / 13.5 / 13.5 vs
    //  10.3 / 10.3 / 11.9; 3584 x 3584 at 64 12.7 / 11.1; 8192 x 4096 at 48 15.9 / 14.5; 12288 x 4096 at 48 19.2 / 18.7, at 64 19.9 / 22.4)
    // (17..32 rows, round 3 with the fragment-major qA image, operator us, tiles vs skinny: N = 8192 15.9 / 12.8, 11008 17.6 / 16.0,
    //  12288 18.8 / 16.0, 18944 x 3584 19.8 / 22.4, 28672 x 8192 41.5 / 49.6: the two-barrier tiles from more than 768 workgroups on.
    //  Callers that pass a row-major image take the same rule: 12288 x 4096 at 32 rows 14.8 skinny vs 15.3 tiles in round 2.)
}

// ---- the ladder: the one place that decides which family a call takes, and in which form --------------------------
// Host only, no device needed (without one num_cus() answers 256).  Every knob is read once here; the launchers read the plan.
GemmPlan plan_gemm(const GemmParams& p, int epi)
{
    GemmPlan pl{};
    const int variant = gemm_variant();
    const bool scratch = p.splitk_ws != nullptr;
    pl.qa_frag = p.a_frag == 1;
    // M <= 16, and M <= 32 on narrow outputs: the weight-streaming GEMV-like kernel (measured against the split-K tiles)
    // ... unless K is long and the tiles are few: then the small tiles with K split over workgroups win (M = 24 / 32 on
    // 4096 x 11008: 14 vs 18 us; on 1024 x 28672: 17 vs 39 us)
    if (takes_skinny(p, epi, variant)) {
        pl.family = GEMM_SKINNY, pl.name = "gemm_skinny_kernel";
        // KW = 4 K-split waves unless a measurement knob says otherwise (40 + kw; 92 + ABL - 1: ablations of the EPI_DEQUANT build, wrong
        // results); the fragment-major qA image has one reader, KW = 4
        const int kw = pl.qa_frag ? 0 : g_skinny_kw.load();
        if (epi == EPI_DEQUANT && kw >= 21 && kw <= 28) pl.skinny_abl = kw <= 24 ? kw - 20 : 7;
        pl.skinny_kw = pl.skinny_abl != 0 || kw < 8 || kw > 16 ? 4 : kw == 16 ? 16 : 8;
        const int mt = (p.M + 15) / 16;
        if (pl.skinny_kw == 4 && pl.skinny_abl == 0 && epi != EPI_INT32) pl.skinny_route = skinny_weight_route(p.a_frag, p.b_image != nullptr, p.M, p.N, p.K);
        const bool image = pl.skinny_route == 1 || pl.skinny_route == 2;
        // (three / four 16-row tiles of qA: 32 features per workgroup on the 256-byte-run route only)
        pl.skinny_tiles = pl.qa_frag && (mt <= 2 || pl.skinny_route == 3) ? skinny_feature_tiles(p.M, p.N, p.K, image) : 1;
        pl.skinny_nt = pl.skinny_route == 3 && skinny_runs_nontemporal(p.N, p.K);
        return pl;
    }
    if (variant == 0 && epi != EPI_INT32 && p.a_frag == 0) {
        const DeepPlan dp = deep_plan(p.M, p.N, p.K);
        if (dp.xs == 1 || (dp.xs > 1 && scratch)) {
            pl.family = GEMM_DEEP, pl.xs = dp.xs;
            // (a forced round-6 schedule on a K that is not whole 128-byte slices: the 8-wave build is what runs)
            pl.deep_build = dp.waves8 == 3 && p.K % KSLICE != 0 ? 1 : dp.waves8;
            pl.deep_early = g_deep_late.load() == 0;
            pl.name = "gemm_w8a8o16_kernel<DEEP> (128x128 tiles, 4 stages in flight, K split over workgroups)";
            if (pl.deep_build == 3) {
                pl.name = "gemm_w8a8o16_mid_kernel<DEEP> (128x128 / 128x96 tiles, copy-only waves, one barrier per pair of slices, K split over workgroups)";
                pl.mid_bn = gemm_mid_tile_width(p.M, p.N, dp.xs);
                pl.mid_rot = gemm_mid_rotated_walk(p.M, dp.xs);
            }
            return pl;
        }
    }
    if (variant >= 100) { // measurement-only ablations of the 256 x 256 ping-pong kernel (last_gemm_kernel keeps its value)
        pl.family = GEMM_PP_ABLATE, pl.cfg = variant - 100;
        return pl;
    }
    auto family = [&pl](int f, const char* name) { return pl.family = f, pl.name = name, pl; };
    if (variant == 0 && gemm_pp128_wins(p.M, p.N, p.K)) return family(GEMM_PP128, "gemm_w8a8o16_pp128_kernel (128x256 ping-pong)");
    if (variant == 0 && epi != EPI_INT32 && scratch) {
        const SplitPlan sp = gemm_splitk_plan(p.M, p.N, p.K);
        pl.xs = sp.s, pl.solo = sp.solo; // 2 / 4 / 8 workgroups per tile
        if (sp.s != 0) return family(GEMM_PP_SPLITK, "gemm_w8a8o16_pp_kernel<SPLITK> (256x256 ping-pong, K split over workgroups)");
    }
    // (measurement / tests) the 128 x 256 ping-pong kernel for every M > 4
    if (variant == 5) return family(GEMM_PP128, "gemm_w8a8o16_pp128_kernel (128x256 ping-pong)");
    const int64_t tiles256 = (int64_t)((p.M + 255) / 256) * ((p.N + 255) / 256);
    const int64_t n64 = (p.N + 63) / 64;
    const int64_t wg32 = (int64_t)((p.M + 31) / 32) * n64, wg64 = (int64_t)((p.M + 63) / 64) * n64;
    if (variant == 2 || (variant == 0 && p.M > 128 && tiles256 >= 96 && wg64 > 768)) return family(GEMM_PP, "gemm_w8a8o16_pp_kernel (256x256 ping-pong)");
    family(GEMM_TILES, "gemm_w8a8o16_kernel (two-barrier tiles)");
    auto tiles = [&pl](int cfg, int bm, int bn, int kgroups) { return pl.cfg = cfg, pl.tile_m = bm, pl.tile_n = bn, pl.kgroups = kgroups, pl; };
    const int force = g_force_cfg.load();
    if (force >= 0 && force < kTileCfgXs32) return tiles(force, 0, 0, 0); // (measurement: described by its number, tile_m == 0)
    // Measured choice (tools/cfg_sweep.sh, M = 32..1024 on 12288x4096, 4096x11008, 4096x4096): small problems are
    // bound by how many workgroups stream operands concurrently, so the 64x64 tile wins until ~3 workgroups per CU.
    // Rule distilled from the sweep: keep ~16 wavefronts on every CU.  With few tiles, several groups of waves share one
    // tile and split K among themselves (KG = 4, then 2); with ~3 tiles per CU plain 64x64 tiles; beyond that 128x128.
    if (epi != EPI_INT32 && scratch) { // few tiles: K split over 2 / 4 workgroups per tile as well
        const XSplitPlan xp = xsplit_plan(p.M, p.N, p.K);
        pl.xs = xp.xs > 1 ? xp.xs : 0;
        if (xp.xs > 1) return tiles(xp.bm == 32 ? kTileCfgXs32 : kTileCfgXs64, xp.bm, 64, 4);
    }
    if (wg32 <= 256) return tiles(22, 32, 64, 4);
    if (wg64 <= 256) return tiles(23, 64, 64, 4);
    if (wg64 <= 512) return tiles(17, 64, 64, 2);
    if (wg64 <= 768) return tiles(7, 64, 64, 1);
    return tiles(4, 128, 128, 1);
}

bool gemm_takes_skinny(const GemmParams& p, int epi) { return plan_gemm(p, epi).family == GEMM_SKINNY; }

// The peer-write epilogue exists for the plain 256 x 256 ping-pong kernel: exactly the shapes whose plan -- automatic selection,
// scratch present, the operator's 128 outlier columns -- is that family; false under any forced schedule.
bool gemm_tp_fused_supported(int M, int N, int K, int O)
{
    if (M <= 128 || N <= 0 || K <= 0 || O < 0 || O > 128 || gemm_variant() != 0) return false;
    static int scratch;
    GemmParams probe{};
    probe.M = M, probe.N = N, probe.K = K, probe.O = 128, probe.splitk_ws = &scratch;
    return plan_gemm(probe, EPI_DEQUANT).family == GEMM_PP;
}

hipError_t launch_gemm(const GemmParams& p, int epi, hipStream_t st, const GemmPlan* planned)
{
    if (p.M <= 0 || p.N <= 0) return hipSuccess;
    if (p.a_frag < 0 || p.a_frag > 2) return hipErrorInvalidValue;
    if (epi_bias(epi) && (p.bias == nullptr || p.Y != nullptr)) return hipErrorInvalidValue; // (no bias form with an addend)
    if (epi_bf16(epi) && (p.Y != nullptr || p.O > 128)) return hipErrorInvalidValue; // (bf16 calls: enqueue's single LDS pass of outliers only)
    if (epi_gate_up(epi) ? (p.n_out <= 0 || p.N != 2 * p.n_out || p.n_out % 16 != 0 || p.Y != nullptr || p.O > 128) : p.n_out != 0)
        return hipErrorInvalidValue; // (merged gate / up: D is [M, N / 2], whole 16-row blocks of the merged weight, no addend)
    const GemmPlan pl = planned ? *planned : plan_gemm(p, epi);
    if (p.a_frag == 1 && pl.family != GEMM_SKINNY) return hipErrorInvalidValue; // (only the skinny kernel reads that image)
    if (p.a_frag == 2 && !(epi == EPI_DEQUANT && pl.family == GEMM_PP)) return hipErrorInvalidValue; // (only the plain 256 x 256 kernel reads that one)
    if (pl.name) note_gemm_kernel(pl.name);
    switch (pl.family) {
    case GEMM_SKINNY: return launch_gemm_skinny(p, epi, pl, st);
    case GEMM_DEEP: return launch_gemm_deep(p, epi, pl, st);
    case GEMM_PP_ABLATE: return launch_gemm_pp_ablate(p, pl.cfg, st);
    case GEMM_PP128: return launch_gemm_pp128(p, epi, st);
    case GEMM_PP_SPLITK: return launch_gemm_pp_splitk(p, epi, pl, st);
    case GEMM_PP: return launch_gemm_pp(p, epi, st);
    default: return launch_gemm_tiles(p, epi, pl, st);
    }
}

// The plan as text (host only).  tests/test_gpu_selection.py launches a grid of shapes and compares the family with last_gemm_kernel();
// tests/golden/selection_table.json pins the answers on BASELINE.json's shapes, so a change of any rule shows up as a diff of that table
// (the rules are tables fitted on measurements -- this makes them readable and reviewable as one).
void describe_gemm_plan(const GemmPlan& pl, char* buf, size_t len)
{
    if (len == 0) return;
    switch (pl.family) {
    case GEMM_SKINNY:
        snprintf(buf, len, "skinny: %d features per workgroup, weight %s, qA %s", 16 * pl.skinny_tiles,
                 pl.skinny_route == 3 ? "row-major in 256-byte runs" : pl.skinny_route == 0 ? "row-major in 64-byte pieces" : "from its registered image",
                 pl.qa_frag ? "fragment-major" : "row-major");
        return;
    case GEMM_DEEP:
        snprintf(buf, len, "deep: 128x%d tiles, %d workgroup(s) per tile along K%s", pl.deep_build == 3 ? pl.mid_bn : 128, pl.xs,
                 pl.deep_build == 3 ? ", copy-only waves" : "");
        return;
    case GEMM_PP_ABLATE: snprintf(buf, len, "ping-pong 256x256 tiles, measurement ablation %d", pl.cfg); return;
    case GEMM_PP128: snprintf(buf, len, "ping-pong 128x256 tiles"); return;
    case GEMM_PP_SPLITK:
        if (pl.solo > 0) snprintf(buf, len, "ping-pong 256x256 tiles: %d whole round(s) solo + tail split %d ways along K", pl.solo / num_cus(), pl.xs);
        else snprintf(buf, len, "ping-pong 256x256 tiles, %d workgroups per tile along K", pl.xs);
        return;
    case GEMM_PP: snprintf(buf, len, "ping-pong 256x256 tiles"); return;
    default: break;
    }
    char kg[24] = "", xs[48] = "";
    if (pl.kgroups > 1) snprintf(kg, sizeof kg, ", %d K groups", pl.kgroups);
    if (pl.xs > 1) snprintf(xs, sizeof xs, ", %d workgroups per tile along K", pl.xs);
    if (pl.tile_m == 0) snprintf(buf, len, "two-barrier tiles, forced configuration %d", pl.cfg);
    else snprintf(buf, len, "two-barrier %dx%d tiles%s%s", pl.tile_m, pl.tile_n, kg, xs);
}

} // namespace mixq
