// The transfer plan of a host-pointer (*_f64) entry point: the rows of the call — what goes up, what comes back, what only lives on
// the device — declared ONCE, in the order they sit in the context's device arena.  One pass (layout) gives every row its offset in
// the arena and its offsets in the pinned staging buffer, and the bytes of both that the call consumes: the sizes HostIo
// (stardis_hip.hip) grows the buffers to and the copies it issues are read from the same rows, so they cannot disagree.
// Plain C++17, no HIP: the host compiler builds it alone (tests/host_plan_probe.cpp).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

struct HostPlan {
    static constexpr size_t kNone = ~(size_t)0;  // "no offset": the row has no such copy, or the call is not staged
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }

    struct Row {
        bool present;      // absent rows (a null host pointer) get a null device address and consume nothing
        const void* src;   // host source of the upload, or null
        void* dst;         // host destination of the download, or null
        size_t bytes;      // bytes on the device (contiguous), and of either copy
        size_t rows;       // the download lands as `rows` rows of bytes / rows each, dst_pitch apart (rows == 1: flat)
        size_t dst_pitch;
        void* slot;        // the caller's pointer variable (a T*) that bind() sets to the device address
        size_t dev_off = kNone, up_off = kNone, down_off = kNone;  // layout(): arena; pinned buffer (uploads first, downloads behind)

        // a present row of zero bytes still has a distinct, valid address
        size_t width() const { return present ? pad(bytes ? bytes : 8) : 0; }
        bool uploads() const { return present && src && bytes; }
        bool downloads() const { return present && dst && bytes; }
    };
    std::vector<Row> rows;
    size_t dev_need = 0, pin_need = 0;  // layout(): the end of the last row in the arena and in the pinned buffer
    bool staged = false;                // layout(): the copies go through the pinned buffer

    // in: uploaded from src
    template <class T> void in(const T* src, size_t bytes, const T** dev) { add(src != nullptr, src, nullptr, bytes, 1, 0, dev); }
    // out: downloaded to dst
    template <class T> void out(T* dst, size_t bytes, T** dev) { add(dst != nullptr, nullptr, dst, bytes, 1, 0, dev); }
    // out, 2-D: n_rows x row_bytes, contiguous on the device, into a host array whose rows are dst_pitch bytes apart
    template <class T> void out2d(T* dst, size_t dst_pitch, size_t row_bytes, size_t n_rows, T** dev)
    {
        const bool flat = dst_pitch == row_bytes || n_rows <= 1;
        add(dst != nullptr, nullptr, dst, row_bytes * n_rows, flat ? 1 : n_rows, flat ? 0 : dst_pitch, dev);
    }
    // inout: uploaded from host and later (if `back`) downloaded to it from the same device buffer
    template <class T> void inout(T* host, size_t bytes, T** dev, bool back = true) { add(host != nullptr, host, back ? host : nullptr, bytes, 1, 0, dev); }
    // scratch: device only
    template <class T> void scratch(size_t bytes, T** dev) { add(true, nullptr, nullptr, bytes, 1, 0, dev); }

    // Offsets and needs of the rows declared so far.  The copies are staged when together they fit staging_max bytes of pinned
    // memory; otherwise they go straight from / to the caller's pages: pin_need is 0 and no row has a pinned offset.
    void layout(size_t staging_max)
    {
        size_t dev = 0, up = 0, down = 0;
        for (Row& r : rows) {
            r.dev_off = r.up_off = r.down_off = kNone;
            if (!r.present) continue;
            r.dev_off = dev, dev += r.width();
            if (r.uploads()) r.up_off = up, up += pad(r.bytes);
            if (r.downloads()) r.down_off = down, down += pad(r.bytes);
        }
        dev_need = dev;
        staged = up + down <= staging_max;
        pin_need = staged ? up + down : 0;
        for (Row& r : rows) {
            if (!staged) r.up_off = r.down_off = kNone;
            if (r.down_off != kNone) r.down_off += up;
        }
    }

    // every row's device address into its caller's variable, for an arena that starts at `base` (after layout())
    void bind(void* base) const
    {
        for (const Row& r : rows) {
            void* p = r.present ? (char*)base + r.dev_off : nullptr;
            std::memcpy(r.slot, &p, sizeof p);  // (the slot is a T* of the caller's: every object pointer has void*'s representation)
        }
    }

private:
    void add(bool present, const void* src, void* dst, size_t bytes, size_t n_rows, size_t dst_pitch, void* slot)
    {
        rows.push_back(Row{present, src, dst, bytes, n_rows, dst_pitch, slot});
    }
};
