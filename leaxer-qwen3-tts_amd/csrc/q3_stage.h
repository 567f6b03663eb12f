// q3_stage.h — host-side bookkeeping that the carried-state stages behind the vocoder share (the pitch stage 4o, the
// stretcher 4m, the tone stage 4r, the loudness stage 4p, the level stage 4n, the PCM sink 4l): the table of open stages with its ids, the counters of each, the refusals of a push and the commit
// of one.  No HIP in here: a stage keeps its device allocation in its own Slot; tests/test_cpu_stage_table.py drives this header from
// a plain g++ harness.  [HINT] no counterpart in the reference, which has no such stage.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace q3 {

constexpr int64_t kStageMaxSamples = 86400000;   // one hour of 24 kHz input per stage

// cur: which half of the stage's double-buffered carry a push reads; it writes the other, and the commit flips them when the stage's
// rule says the push left a carry
struct StageSlot { bool used = false, finished = false; int cur = 0; int64_t n_in = 0, n_out = 0; };

// Slot: StageSlot plus the stage's own parameters and allocation, which outlive end() for the id's next owner.  Err: what a refusal
// throws, constructed from the text.  name / noun / none: the kind's words in the refusals, "<name>: <noun> 3 is finished", "<name>: <none>"
template <class Slot, class Err>
struct StageTable {
    const char *name, *noun, *none;
    int max;                                    // open at the same time
    std::vector<Slot> slots;

    std::string who(int id) const { return std::string(name) + ": " + noun + " " + std::to_string(id); }
    int free_id() {                             // the lowest id that is not open; the table grows by one when all are
        for (size_t i = 0; i < slots.size(); ++i) if (!slots[i].used) return (int)i;
        if ((int)slots.size() >= max) throw Err(std::string(name) + ": at most " + std::to_string(max) + " " + noun + "s are open at a time");
        slots.emplace_back();
        return (int)slots.size() - 1;
    }
    Slot& open(int id) {                        // after the stage's own checks and allocations for free_id()'s id: nothing before it marks the id
        StageSlot& S = slots[(size_t)id];
        S.used = true; S.finished = false; S.cur = 0; S.n_in = S.n_out = 0;
        return slots[(size_t)id];
    }
    const Slot& get(int id) const {
        if (id < 0 || id >= (int)slots.size() || !slots[(size_t)id].used) throw Err(std::string(name) + ": " + none);
        return slots[(size_t)id];
    }
    void end(int id) { (void)get(id); slots[(size_t)id].used = false; }
    // samples a push of n_new more would deliver, by the stage's rule emitted(slot, samples received, finish); throws when the push
    // would be refused.  Changes nothing.
    template <class Rule>
    int64_t push_len(int id, int64_t n_new, bool finish, Rule emitted) const {
        const Slot& S = get(id);
        if (S.finished) throw Err(who(id) + " is finished");
        if (n_new < 0) throw Err(std::string(name) + ": negative sample count");
        if (S.n_in + n_new > kStageMaxSamples) throw Err(who(id) + " would exceed one hour of 24 kHz input");
        return emitted(S, S.n_in + n_new, finish) - S.n_out;
    }
    void commit(int id, int64_t n_new, int64_t n_out, bool finish, bool flip) {   // a completed push
        StageSlot& S = slots[(size_t)id];
        if (flip) S.cur = 1 - S.cur;
        S.n_in += n_new; S.n_out += n_out;
        if (finish) S.finished = true;
    }
};

} // namespace q3
