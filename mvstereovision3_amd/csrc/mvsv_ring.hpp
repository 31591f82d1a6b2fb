// mvsv_ring.hpp — slot bookkeeping of the frame stream (mvsv_stream.cpp), kept
// free of HIP so the CPU suite can drive it under AddressSanitizer + UBSan.
//
// Frames are numbered by push order; frame f lives in slot f % depth.  head =
// frames pushed, tail = frames popped, launched = frames whose compute is
// enqueued (tail <= launched <= head, head - tail <= depth).  Pushed frames are
// launched as runs of consecutive slots; a run never wraps past the ring's end,
// so its slots are one contiguous [frame][H][W] block of the device arrays.
// Also here, for the same reason: where the frames of a batched device push go
// (ring_push_segments), which source pointers such a push accepts (ring_source_ok),
// the layout of a stage's pinned slot (ring_slot_block) and the geometry of a push
// of each kind (ring_push_geom).
#pragma once

#include <algorithm>
#include <cstddef>

namespace mvsv {

struct RingRun {
    long i0;  // first slot
    int n;    // slots
};

// The next run to launch, or false when every pushed frame is launched.
inline bool ring_next_run(long launched, long head, long depth, RingRun* r)
{
    if (launched >= head) return false;
    r->i0 = launched % depth;
    r->n = (int)std::min(head - launched, depth - r->i0);
    return true;
}

// After a push: launch when a full group of `batch` frames is pending, or when
// the group would otherwise wrap past the ring's end.
inline bool ring_launch_after_push(long head, long launched, int batch, long depth)
{
    return head - launched >= batch || head % depth == 0;
}

inline bool ring_full(long head, long tail, long depth) { return head - tail >= depth; }

// The slots that n consecutive pushes starting at frame `head` fill, as at most
// two pieces of consecutive slots (the second starts at slot 0 after the ring's
// end).  Returns the number of pieces; 0 unless 1 <= n <= depth.  That the slots
// are free (n <= depth - pending) is the caller's check.
inline int ring_push_segments(long head, int n, long depth, RingRun out[2])
{
    if (n < 1 || n > depth) return 0;
    const long i0 = head % depth;
    const int first = (int)std::min<long>(n, depth - i0);
    out[0] = RingRun{i0, first};
    if (first == n) return 1;
    out[1] = RingRun{0, n - first};
    return 2;
}

// Where the source of a device push may live (mvsv_stream_push_device): what
// hipPointerGetAttributes reports, restated without HIP types.
enum PtrKind {
    kPtrUnregistered = 0,  // pageable host memory the runtime does not know
    kPtrHost = 1,          // pinned / registered host memory
    kPtrDevice = 2,
    kPtrManaged = 3,
    kPtrOther = 4,  // arrays and whatever else the runtime may name
};

// query_ok: the attribute query succeeded.  ptr_device: the device the
// allocation belongs to.  device_ptr: the query reported a device-side address.
// Accepted: memory of the stream's device, and host memory that its kernels can
// read (pinned with a device address, or managed).
inline bool ring_source_ok(bool query_ok, PtrKind kind, int ptr_device, int stream_device, bool device_ptr)
{
    if (!query_ok) return false;
    switch (kind) {
    case kPtrDevice: return ptr_device == stream_device;
    case kPtrHost: return device_ptr;
    case kPtrManaged: return true;
    default: return false;
    }
}

// One slot of a stage's pinned host block: three parts one after the other, the
// second aligned to mid_align (a power of two), the slot padded to 16 bytes.
// An image stage keeps (image | int16 min, max | nothing), mid_align 2; the sample
// points keep (float values | int count | hit records), mid_align 4.
struct SlotBlock {
    size_t mid = 0, tail = 0;  // offsets of the second and the third part
    size_t bytes = 0;          // from one slot to the next
};

inline SlotBlock ring_slot_block(size_t first_bytes, size_t mid_align, size_t mid_bytes, size_t tail_bytes)
{
    SlotBlock b;
    b.mid = (first_bytes + mid_align - 1) & ~(mid_align - 1);
    b.tail = b.mid + mid_bytes;
    b.bytes = (b.tail + tail_bytes + 15) & ~(size_t)15;
    return b;
}

// What a push copies and where it lands in a slot's staging and device buffers,
// which share one layout: `rows` rows of `row` bytes per image, `stride` bytes
// apart.  right != 0: the pair is one buffer, the right image `right` bytes after
// the left; right == 0: two buffers (the matcher's own input arrays).  `frame`:
// bytes from one slot's device buffer(s) to the next slot's.
enum PushKind { kPushRectified, kPushRaw, kPushBgr };

struct PushGeom {
    int rows;
    size_t row, stride, right, frame;
};

// W x H: the stream's (rectified) size; rawW x rawH: a raw stream's camera frame;
// bgrW x bgrH: the colour frame, its staged rows padded to 4 bytes (packed loads).
inline PushGeom ring_push_geom(PushKind kind, int W, int H, int rawW, int rawH, int bgrW, int bgrH)
{
    PushGeom g{};
    if (kind == kPushRaw) {
        g.rows = rawH;
        g.row = g.stride = (size_t)rawW;
        g.right = g.stride * g.rows;
        g.frame = 2 * g.right;
    } else if (kind == kPushBgr) {
        g.rows = bgrH;
        g.row = 3 * (size_t)bgrW;
        g.stride = (g.row + 3) & ~(size_t)3;
        g.right = g.stride * g.rows;
        g.frame = 2 * g.right;
    } else {
        g.rows = H;
        g.row = g.stride = (size_t)W;
        g.frame = g.stride * g.rows;
    }
    return g;
}

}  // namespace mvsv
