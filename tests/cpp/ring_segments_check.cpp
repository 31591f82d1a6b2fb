// ring_push_segments and ring_source_ok (mvsv_ring.hpp, HIP-free), exhaustively for
// small rings.  A batched device push of n frames must fill the slots, and launch the
// runs, that n single pushes fill and launch: the pieces are replayed against
// ring_launch_after_push / ring_next_run.  Built stand-alone, with ASan + UBSan.
#include <cstdio>
#include <vector>

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

int main()
{
    check_segments();
    check_sources();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
