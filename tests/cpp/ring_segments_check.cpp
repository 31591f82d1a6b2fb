// ring_push_segments and ring_source_ok (mvsv_ring.hpp, HIP-free), exhaustively for
// small rings.  A batched device push of n frames must fill the slots, and launch the
// runs, that n single pushes fill and launch: the pieces are replayed against
// ring_launch_after_push / ring_next_run.  Also the layout of a stage's pinned slot
// (ring_slot_block) and the geometry of the pushes (ring_push_geom) against the
// formulas and values they replaced.  Built stand-alone, with ASan + UBSan.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../include/mvsv.h"
#include "mvsv_ring.hpp"

using namespace mvsv;

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            failures++;                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
        }                                                                     \
    } while (0)

// the runs that launching after every push (and once at the end) produces
static std::vector<RingRun> replay(long head, long launched, int n, int batch, long depth, std::vector<long>* slots)
{
    std::vector<RingRun> runs;
    for (int k = 0; k < n; k++) {
        slots->push_back(head % depth);
        head++;
        if (ring_launch_after_push(head, launched, batch, depth)) {
            RingRun r;
            while (ring_next_run(launched, head, depth, &r)) {
                runs.push_back(r);
                launched += r.n;
            }
        }
    }
    return runs;
}

static void check_segments()
{
    long cases = 0;
    for (long depth = 1; depth <= 6; depth++)
        for (long head = 0; head < 3 * depth; head++)
            for (int n = -1; n <= depth + 1; n++) {
                RingRun seg[2] = {{-1, -1}, {-1, -1}};
                const int pieces = ring_push_segments(head, n, depth, seg);
                cases++;
                if (n < 1 || n > depth) {
                    CHECK(pieces == 0);
                    continue;
                }
                CHECK(pieces == 1 || pieces == 2);
                // contiguous, in order, inside the ring, summing to n
                std::vector<long> got;
                for (int g = 0; g < pieces; g++) {
                    CHECK(seg[g].n >= 1 && seg[g].i0 >= 0 && seg[g].i0 + seg[g].n <= depth);
                    for (int k = 0; k < seg[g].n; k++) got.push_back(seg[g].i0 + k);
                }
                CHECK((long)got.size() == n);
                CHECK(seg[0].i0 == head % depth);
                if (pieces == 2) CHECK(seg[0].i0 + seg[0].n == depth && seg[1].i0 == 0);
                // the slots of n single pushes, for every batch and every launched <= head
                for (int batch = 1; batch <= depth; batch++)
                    for (long pend = 0; pend + n <= depth && pend <= head; pend++) {
                        // unlaunched frames never reach back over the ring's end
                        const long launched = head - std::min(pend, head % depth);
                        std::vector<long> slots;
                        const std::vector<RingRun> runs = replay(head, launched, n, batch, depth, &slots);
                        CHECK(slots == got);
                        // every run ends inside one piece: at its last slot or where a launch fell due
                        for (const RingRun& r : runs) {
                            CHECK(r.n >= 1 && r.i0 + r.n <= depth);
                            const long end = r.i0 + r.n - 1;
                            bool inside = false;
                            for (int g = 0; g < pieces; g++)
                                inside = inside || (end >= seg[g].i0 && end < seg[g].i0 + seg[g].n);
                            CHECK(inside);
                        }
                        // a push that reaches the ring's end leaves nothing of it unlaunched
                        if (pieces == 2) {
                            long covered = 0;
                            for (const RingRun& r : runs) covered += r.n;
                            CHECK(covered >= (head - launched) + seg[0].n);
                        }
                    }
            }
    std::printf("segments: %ld cases\n", cases);
}

static void check_sources()
{
    long cases = 0;
    for (int ok = 0; ok <= 1; ok++)
        for (int kind = kPtrUnregistered; kind <= kPtrOther; kind++)
            for (int pdev = -1; pdev <= 2; pdev++)
                for (int sdev = 0; sdev <= 2; sdev++)
                    for (int dptr = 0; dptr <= 1; dptr++) {
                        bool want = false;
                        if (ok) {
                            if (kind == kPtrDevice) want = pdev == sdev;
                            if (kind == kPtrHost) want = dptr != 0;
                            if (kind == kPtrManaged) want = true;
                        }
                        CHECK(ring_source_ok(ok != 0, (PtrKind)kind, pdev, sdev, dptr != 0) == want);
                        cases++;
                    }
    // the plain cases, spelled out
    CHECK(ring_source_ok(true, kPtrDevice, 0, 0, true));
    CHECK(!ring_source_ok(true, kPtrDevice, 1, 0, true));
    CHECK(!ring_source_ok(true, kPtrUnregistered, 0, 0, false));
    CHECK(!ring_source_ok(false, kPtrDevice, 0, 0, true));
    CHECK(ring_source_ok(true, kPtrHost, 0, 0, true));
    CHECK(!ring_source_ok(true, kPtrHost, 0, 0, false));
    CHECK(!ring_source_ok(true, kPtrOther, 0, 0, true));
    std::printf("sources: %ld cases\n", cases);
}

static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ring_slot_block against the formulas the stream used for its pinned slots
// (disp_minmax / view_minmax: the image padded to 2 bytes, two int16, the slot
// padded to 16; sp_count / sp_hits: values, one int, the hit records, padded to 16).
static void check_slot_blocks()
{
    long cases = 0;
    for (size_t bytes : {(size_t)0, (size_t)1, (size_t)2, (size_t)15, (size_t)16, (size_t)17, (size_t)651}) {
        const SlotBlock b = ring_slot_block(bytes, alignof(int16_t), 2 * sizeof(int16_t), 0);
        // restated: minmax at (bytes + 1) & ~1, slot (that + 4 + 15) & ~15
        const size_t mm = (bytes + 1) & ~(size_t)1;
        CHECK(b.mid == mm);
        CHECK(b.tail == mm + 4);
        CHECK(b.bytes == ((mm + 2 * sizeof(int16_t) + 15) & ~(size_t)15));
        CHECK(b.mid >= bytes);                      // the image ends before (min, max)
        CHECK(b.mid % alignof(int16_t) == 0);       // int16 aligned (slots start 16-aligned)
        CHECK(b.mid + 2 * sizeof(int16_t) <= b.bytes);  // (min, max) ends inside the slot
        CHECK(b.bytes % 16 == 0);                   // slot i + 1 starts at or after slot i's end, aligned
        CHECK(b.bytes == up(b.mid + 4, 16));
        cases++;
    }
    for (int npts : {0, 5})
        for (int max_hits : {1, 5}) {
            const size_t hit = sizeof(mvsv_sample_hit);
            const SlotBlock b = ring_slot_block((size_t)npts * sizeof(float), alignof(int), sizeof(int),
                                                (size_t)max_hits * hit);
            // restated: count = values + npts floats, hits = count + 1 int,
            // slot = (npts * 4 + 4 + max_hits * sizeof(hit) + 15) & ~15
            CHECK(b.mid == (size_t)npts * sizeof(float));
            CHECK(b.tail == (size_t)npts * sizeof(float) + sizeof(int));
            CHECK(b.bytes == (((size_t)npts * sizeof(float) + sizeof(int) + (size_t)max_hits * hit + 15) & ~(size_t)15));
            CHECK(b.mid >= (size_t)npts * sizeof(float) && b.tail >= b.mid + sizeof(int));  // no overlap
            CHECK(b.tail + (size_t)max_hits * hit <= b.bytes);
            CHECK(b.mid % alignof(int) == 0);
            CHECK(b.tail % alignof(mvsv_sample_hit) == 0);
            CHECK(b.bytes % 16 == 0);
            cases++;
        }
    std::printf("slot blocks: %ld cases\n", cases);
}

// ring_push_geom against the literal values of the three host pushes and of the
// device push's geometry chain: a 17 x 5 stream, raw frame, colour frame, and a
// 5-wide colour frame (row 15, staged stride 16).
static void check_push_geom()
{
    // rectified pairs: W-byte rows into dL / dR (two arrays), frame stride W * H
    PushGeom g = ring_push_geom(kPushRectified, 17, 5, 0, 0, 0, 0);
    CHECK(g.rows == 5 && g.row == 17 && g.stride == 17 && g.right == 0 && g.frame == 85);
    // raw pairs: [2][rawH][rawW] per slot; the stream's own size plays no part
    g = ring_push_geom(kPushRaw, 9, 3, 17, 5, 0, 0);
    CHECK(g.rows == 5 && g.row == 17 && g.stride == 17 && g.right == 85 && g.frame == 170);
    // colour pairs: rows of 3 * 17 = 51 bytes staged 52 apart, [2][bgrH][52] per slot
    g = ring_push_geom(kPushBgr, 9, 3, 0, 0, 17, 5);
    CHECK(g.rows == 5 && g.row == 51 && g.stride == 52 && g.right == 260 && g.frame == 520);
    g = ring_push_geom(kPushBgr, 5, 5, 0, 0, 5, 5);
    CHECK(g.rows == 5 && g.row == 15 && g.stride == 16 && g.right == 80 && g.frame == 160);
    // the kinds index the host pushes' message table
    CHECK(kPushRectified == 0 && kPushRaw == 1 && kPushBgr == 2);
    std::printf("push geometry: 4 cases\n");
}

int main()
{
    check_segments();
    check_sources();
    check_slot_blocks();
    check_push_geom();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
