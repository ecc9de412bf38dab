// plade_amd/csrc/work_slot.h -- the owner of one tool's work area inside a plade_ctx.  No HIP and no project include, so that it
// can be tested on its own (tests/cxx/work_slot_harness.cpp).
#pragma once

namespace plade {

// A type-erased owning pointer.  The context holds one per tool and never sees the tool's work struct; the tool's .hip file, where
// the struct is complete, creates it on first use (work_in) and installs the deleter with it.
struct WorkSlot {
    void *p = nullptr;
    void (*del)(void *) = nullptr;
    WorkSlot() = default;
    WorkSlot(const WorkSlot &) = delete;
    WorkSlot &operator=(const WorkSlot &) = delete;
    ~WorkSlot() { reset(); }
    void reset() {   // idempotent
        if (p) del(p);
        p = nullptr;
    }
};

// the slot's W, made on first use (a slot holds one type for life; two slots of one type are two objects)
template <class W>
W &work_in(WorkSlot &s) {
    if (!s.p) {
        s.p = new W;
        s.del = [](void *q) { delete static_cast<W *>(q); };
    }
    return *static_cast<W *>(s.p);
}

}  // namespace plade
