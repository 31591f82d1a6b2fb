// stage_layout_check.cpp — the staging layouts of the host-pointer calls
// (mvstereovision3_amd/csrc/mvsv_stage.hpp, its HIP-free part), through the very
// structs the entry points reserve with.  For every call and a grid of sizes:
// the slices are disjoint, inside the total and 256-byte aligned; every pitch
// covers its row and keeps its stated alignment, and is the pitch the call staged
// with before there was an arena; and the arena is no larger than the three
// buffers that call used to ask for, plus 256 bytes of padding per slice.
// The old sizes are written out as formulas, each with the line of commit 1dbbb3f
// ("GPU parity tests for kernel forms only switches and full frames reach") it was
// read from.  Built stand-alone with ASan + UBSan, no library, no GPU.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <set>
#include <string>

#include "mvsv_stage.hpp"

using namespace mvsv;

static int failures = 0;
static long cases = 0;
static std::set<std::string> calls;  // the entry points whose reservation was checked
#define CHECK(c)                                                                            \
    do {                                                                                    \
        if (!(c)) {                                                                         \
            failures++;                                                                     \
            std::printf("FAIL %s:%d: %s (%s %d x %d)\n", __FILE__, __LINE__, #c, g_call, g_w, g_h); \
        }                                                                                   \
    } while (0)

static const char* g_call = "";
static int g_w = 0, g_h = 0;

// what holds for every layout; old_bytes: what the call's buffers added up to
static void check_layout(const char* call, const StageLayout& lay, size_t old_bytes)
{
    g_call = call;
    cases++;
    calls.insert(call);
    CHECK(lay.count >= 2 && lay.count <= kStageMaxSlices);
    CHECK(lay.total % kStageAlign == 0);
    for (int i = 0; i < lay.count; i++) {
        const StageSlice& a = lay.slice[i];
        CHECK(a.off % kStageAlign == 0);
        CHECK(a.off + a.bytes <= lay.total);
        CHECK(a.pitch >= a.row_bytes);
        CHECK(a.row_align > 0 && a.pitch % a.row_align == 0);
        CHECK(a.pitch - a.row_bytes < a.row_align);  // no more padding than the alignment asks for
        CHECK(a.pitch == 0 ? a.bytes == 0 : a.bytes % a.pitch == 0);
        for (int j = 0; j < i; j++) {
            const StageSlice& b = lay.slice[j];
            CHECK(a.off + a.bytes <= b.off || b.off + b.bytes <= a.off);
        }
    }
    CHECK(lay.total <= old_bytes + kStageAlign * (size_t)lay.count);
}

static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static void check_size(int Wi, int Hi)
{
    g_w = Wi;
    g_h = Hi;
    const size_t W = Wi, H = Hi, px = W * H;
    const size_t ws8 = up(W, 8);  // "const size_t ws = ((size_t)W + 7) & ~(size_t)7"

    // mvsv_sgbm, mvsv_sgbm_bgr, mvsv_bm -- mvsv_host.cpp:940-944: ib = W * cn * H twice, fb * 2
    const char* pair_names[3] = {"mvsv_sgbm", "mvsv_sgbm_bgr", "mvsv_bm"};
    const size_t pair_cn[3] = {1, 3, 1};
    for (int k = 0; k < 3; k++) {
        const size_t cn = pair_cn[k];
        const PairStage s(W, H, cn, 2);
        check_layout(pair_names[k], s, 2 * (W * cn * H) + px * 2);
        CHECK(s.left.pitch == W * cn && s.right.pitch == W * cn && s.out.pitch == W * 2);  // :946-954
        CHECK(s.left.bytes == W * cn * H && s.out.bytes == px * 2);
    }
    {  // mvsv_tm -- mvsv_tm.hip:275-278: px three times
        const PairStage s(W, H, 1, 1);
        check_layout("mvsv_tm", s, 3 * px);
        CHECK(s.left.pitch == W && s.right.pitch == W && s.out.pitch == W);  // :281-287
    }
    // SamplepointDetection's lattice -- mvsv_post.hip:1344-1348
    const size_t nx = W / 8 ? W / 8 - 1 : 0, ny = H / 8 ? H / 8 - 1 : 0, lattice = nx * ny;
    {  // mvsv_mean_disparity_grid -- mvsv_stream.cpp:1635-1637: px * 2 + 4 + 81 floats
        const MapFloatsStage s(W, H, 81);
        check_layout("mvsv_mean_disparity_grid", s, px * 2 + 4 + 81 * sizeof(float));
        CHECK(s.map.pitch == W * 2 && s.floats.bytes == 81 * sizeof(float));  // :1641-1644
    }
    for (size_t npts : {lattice, (size_t)1, px}) {  // mvsv_samplepoint_values -- mvsv_host.cpp:770-772
        const MapFloatsStage s(W, H, npts);
        check_layout("mvsv_samplepoint_values", s, px * 2 + 4 + npts * sizeof(float));
        CHECK(s.map.pitch == W * 2 && s.floats.bytes == npts * sizeof(float));  // :776-779
    }
    {  // mvsv_normalize_minmax -- mvsv_host.cpp:831-833: px = ws * H, px * 3 + 4
        const NormalizeStage s(W, H);
        check_layout("mvsv_normalize_minmax", s, ws8 * H * 3 + 4);
        CHECK(s.map.pitch == ws8 * 2 && s.out.pitch == ws8);  // :838-841
        CHECK(s.map.bytes == ws8 * H * 2 && s.out.bytes == ws8 * H);
    }
    for (size_t npts : {(size_t)0, lattice}) {
        // mvsv_view -- mvsv_host.cpp:885-890: px * 2 + ob + 16 + (81 + npts) floats, ob = 3 W H up to 16
        const ViewStage s(W, H, npts);
        check_layout("mvsv_view", s, ws8 * H * 2 + up(3 * px, 16) + 16 + (81 + npts) * sizeof(float));
        CHECK(s.map.pitch == ws8 * 2 && s.out.pitch == 3 * W);  // :900-908
        CHECK(s.means.bytes == 81 * sizeof(float) && s.values.bytes == npts * sizeof(float));
    }
    const char* cloud_names[2] = {"mvsv_point_cloud", "mvsv_dmap2pcl"};
    for (size_t capacity : {(size_t)1, px / 2 + 1, px, (size_t)INT_MAX})
        for (int k = 0; k < 2; k++) {
            // mvsv_host.cpp:1012-1016: px * 2 + 3 ints (px = ws * H), cap records of 16 bytes,
            // cap = min(capacity, W * H); mvsv_dmap2pcl passes INT32_MAX (:1068)
            const size_t asked = k == 1 ? (size_t)INT_MAX : capacity, cap = std::min(asked, px);
            const CloudStage s(W, H, asked);
            check_layout(cloud_names[k], s, ws8 * H * 2 + 3 * sizeof(int) + cap * 16);
            CHECK(s.map.pitch == ws8 * 2 && s.records.bytes == cap * 16 && s.header.bytes == 12);  // :1020-1024
        }
    for (size_t dw : {(size_t)1, (W + 1) / 2, 2 * W})
        for (size_t dh : {(size_t)1, (H + 1) / 2, 2 * H}) {
            {  // mvsv_resize -- mvsv_host.cpp:1126-1129: sw * sh and dw * dh
                const ImageStage s(H, W, kRowTight, dw, dh);
                check_layout("mvsv_resize", s, px + dw * dh);
                CHECK(s.in.pitch == W && s.out.pitch == dw);  // :1132-1136
            }
            {  // mvsv_prepare_gray -- mvsv_host.cpp:1173-1176: drow * sh and dw * dh, drow = 3 sw up to 4
                const ImageStage s(H, 3 * W, kRow4, dw, dh);
                check_layout("mvsv_prepare_gray", s, up(3 * W, 4) * H + dw * dh);
                CHECK(s.in.pitch == up(3 * W, 4) && s.in.row_bytes == 3 * W && s.out.pitch == dw);  // :1179-1183
            }
        }
    {  // mvsv_rectify_pair -- mvsv_host.cpp:1205-1209: 2 px, 2 px, 4 px floats
        const RemapStage s(W, H, 4 * px);
        check_layout("mvsv_rectify_pair", s, 2 * px + 2 * px + 4 * px * sizeof(float));
        CHECK(s.src.pitch == W && s.dst.pitch == W && s.src.bytes == 2 * px && s.dst.bytes == 2 * px);  // :1218-1234
        CHECK(s.src.off != s.dst.off && s.maps.bytes == 4 * px * sizeof(float));
    }
    {  // mvsv_sharpness -- mvsv_host.cpp:1273-1275: sum_at + 8, sum_at = (ws * H) up to 8, ws = W up to 4
        const SharpnessStage s(W, H);
        check_layout("mvsv_sharpness", s, up(up(W, 4) * H, 8) + 8);
        CHECK(s.img.pitch == up(W, 4) && s.sum.bytes == 8);  // :1279-1281
    }
    {  // mvsv_undistort_pair -- mvsv_host.cpp:1318-1321: 2 px and 2 px (the maps are cached apart)
        const RemapStage s(W, H, 0);
        check_layout("mvsv_undistort_pair", s, 2 * px + 2 * px);
        CHECK(s.src.pitch == W && s.dst.pitch == W && s.src.bytes == 2 * px && s.dst.bytes == 2 * px);  // :1358-1366
        CHECK(s.src.off != s.dst.off && s.maps.bytes == 0);  // in-place calls stay safe
    }
}

int main()
{
    for (int W : {1, 3, 4, 7, 8, 9, 37, 640, 1281})
        for (int H : {1, 2, 23}) check_size(W, H);
    std::printf("calls:");
    for (const std::string& c : calls) std::printf(" %s", c.c_str());
    std::printf("\nlayouts: %ld checked, %zu calls, %d failures\n", cases, calls.size(), failures);
    return failures ? 1 : 0;
}
