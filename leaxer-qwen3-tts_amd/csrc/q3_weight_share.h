// q3_weight_share.h — host-only bookkeeping of a weight set that several engines hold ("The weight set").
// No HIP call: tools/weight_share_sanitize.cpp runs it under ASan / UBSan / TSan without a GPU.  q3_engine.h's WeightSet derives
// from ShareBook and adds the device memory.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>

namespace q3 {

// Who holds the set, whether it may be handed to one more holder, and which calls a shared set refuses.  Every field is read and written
// under mu; build_mu serialises the one derived piece that a later holder may add (the layer-0 QKV table).
struct ShareBook {
    mutable std::mutex mu;
    std::mutex build_mu;
    int holders = 0;          // engines that hold the set
    bool published = false;   // finalize's device work has completed: the set may be joined
    int64_t bytes = 0;        // HBM the set holds (registry + derived copies)

    void hold() { std::lock_guard<std::mutex> lk(mu); ++holders; }                   // the creating engine
    bool join() { std::lock_guard<std::mutex> lk(mu); if (!published) return false; ++holders; return true; }   // a sharer: only a published set
    int leave() { std::lock_guard<std::mutex> lk(mu); return --holders; }
    int n_holders() const { std::lock_guard<std::mutex> lk(mu); return holders; }
    bool is_published() const { std::lock_guard<std::mutex> lk(mu); return published; }
    void publish(bool on) { std::lock_guard<std::mutex> lk(mu); published = on; }
    void add_bytes(int64_t n) { std::lock_guard<std::mutex> lk(mu); bytes += n; }
    int64_t n_bytes() const { std::lock_guard<std::mutex> lk(mu); return bytes; }
    // set_tensor / fill_synthetic / load_weights: empty when allowed, else the refusal's text
    std::string mutation_refusal() const {
        std::lock_guard<std::mutex> lk(mu);
        return holders > 1 ? "weights are shared by " + std::to_string(holders) + " engines" : std::string();
    }
    // finalize on a published set that others hold too: nothing to do (and nothing may be rebuilt under them)
    bool finalize_is_noop() const { std::lock_guard<std::mutex> lk(mu); return published && holders > 1; }
    // The piece that is built at most once by the first holder it applies to.  `have` says whether it exists, `build` makes it, leaves
    // its device work completed and returns its bytes.  Returns true when this call built it.
    template <class Have, class Build> bool build_once(Have&& have, Build&& build) {
        std::lock_guard<std::mutex> lk(build_mu);
        if (have()) return false;
        const int64_t n = build();
        add_bytes(n);
        return true;
    }
};

// An engine's hold on a set: counted from construction (also when the engine's constructor throws later) until destruction; the last
// one to leave destroys the set.
template <class Set> struct SetHold {
    std::shared_ptr<Set> set;
    explicit SetHold(std::shared_ptr<Set> s) : set(std::move(s)) {}
    SetHold(const SetHold&) = delete;
    SetHold& operator=(const SetHold&) = delete;
    ~SetHold() { if (set) set->leave(); }
};

} // namespace q3
