// dev_buf.hpp -- the one owner of a device array taken from a handle's pool (engine_state.hip.hpp: dev_alloc fills it, dev_free takes the block
// back).  Host-only, nothing of HIP in here: the release goes through dev_buf_release, which the engine defines as dev_free and
// tests/test_dev_buf_host.py as a recording stub.
#pragma once
#include <utility>

void dev_buf_release(void* p);

// Move-only; empty by default; releases its block when destroyed, reset or assigned to.  Converts to T*: launch sites, pointer arithmetic and
// null tests read as with a plain pointer.  Second state, for gmg_dist_bind alone: borrow(p) holds a pointer somebody else owns -- never released.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), borrowed_(o.borrowed_) { o.p_ = nullptr; o.borrowed_ = false; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; borrowed_ = o.borrowed_; o.p_ = nullptr; o.borrowed_ = false; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p_ && !borrowed_) dev_buf_release(p_);
        p_ = nullptr; borrowed_ = false;
    }
    void adopt(T* fresh) { reset(); p_ = fresh; }                     // a block just taken from the pool (dev_alloc)
    void borrow(T* external) { reset(); p_ = external; borrowed_ = external != nullptr; }
    bool borrowed() const { return borrowed_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
    bool borrowed_ = false;
};
