// weight_share_sanitize.cpp — the host-only bookkeeping of a shared weight set (csrc/q3_weight_share.h: ShareBook, SetHold) under
// AddressSanitizer + UBSan, and under ThreadSanitizer: holder counting, the refusals of a shared set, lifetimes in any order, the
// build-once rule of the late piece, all from several threads.  No GPU, no HIP call: tools/weight_share_sanitize.sh builds and runs it.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "q3_weight_share.h"

using q3::SetHold;
using q3::ShareBook;

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

// stands in for WeightSet: what it owns is freed by the last holder, exactly once
struct FakeSet : ShareBook {
    static std::atomic<int> live, freed;
    std::vector<int>* payload = new std::vector<int>(1024, 7);
    int* table = nullptr;
    FakeSet() { live.fetch_add(1); }
    ~FakeSet() { delete payload; delete[] table; live.fetch_sub(1); freed.fetch_add(1); }
};
std::atomic<int> FakeSet::live{0}, FakeSet::freed{0};

static std::shared_ptr<FakeSet> fresh(bool publish) {
    auto s = std::make_shared<FakeSet>();
    s->hold();
    s->add_bytes(4096);
    if (publish) s->publish(true);
    return s;
}

// what Engine's constructor does with a donor's set: null when the set cannot be joined
static std::unique_ptr<SetHold<FakeSet>> share(const std::shared_ptr<FakeSet>& s) {
    if (!s->join()) return nullptr;
    return std::unique_ptr<SetHold<FakeSet>>(new SetHold<FakeSet>(s));
}

static void rules() {
    auto set = fresh(false);
    std::unique_ptr<SetHold<FakeSet>> donor(new SetHold<FakeSet>(set));
    set.reset();
    FakeSet& s = *donor->set;
    CHECK(s.n_holders() == 1 && s.mutation_refusal().empty() && !s.finalize_is_noop());
    CHECK(share(donor->set) == nullptr && s.n_holders() == 1);      // not finalized: refused, nothing counted
    s.publish(true);
    CHECK(!s.finalize_is_noop());                                    // alone: finalize rebuilds as before
    auto a = share(donor->set), b = share(donor->set);
    CHECK(a && b && s.n_holders() == 3);
    CHECK(s.mutation_refusal() == "weights are shared by 3 engines" && s.finalize_is_noop());
    CHECK(s.n_bytes() == 4096);
    int built = 0;
    for (int i = 0; i < 3; ++i)
        built += s.build_once([&] { return s.table != nullptr; }, [&]() -> int64_t { s.table = new int[16](); return 64; }) ? 1 : 0;
    CHECK(built == 1 && s.n_bytes() == 4096 + 64);
    bool threw = false;
    FakeSet& other = *a->set;
    delete[] other.table; other.table = nullptr;
    try { other.build_once([&] { return other.table != nullptr; }, [&]() -> int64_t { throw 1; }); } catch (int) { threw = true; }
    CHECK(threw && other.n_bytes() == 4096 + 64);                    // a failed build counts nothing and leaves the mutex free
    CHECK(other.build_once([&] { return other.table != nullptr; }, [&]() -> int64_t { other.table = new int[16](); return 0; }));
    donor.reset();                                                   // the donor goes first
    CHECK(FakeSet::live.load() == 1 && a->set->n_holders() == 2 && a->set->payload->at(5) == 7);
    b.reset();
    CHECK(a->set->n_holders() == 1 && a->set->mutation_refusal().empty() && !a->set->finalize_is_noop());   // a sharer alone may mutate again
    a->set->publish(false);                                          // set_tensor
    CHECK(share(a->set) == nullptr);
    a.reset();
    CHECK(FakeSet::live.load() == 0 && FakeSet::freed.load() == 1);
}

// a holder whose constructor throws behind the hold leaves the count as it was
static void throwing_holder() {
    auto set = fresh(true);
    SetHold<FakeSet> donor(set);
    struct Engine { SetHold<FakeSet> hold; explicit Engine(std::shared_ptr<FakeSet> s) : hold(std::move(s)) { throw 2; } };
    bool threw = false;
    CHECK(set->join());
    try { Engine e(set); } catch (int) { threw = true; }
    CHECK(threw && set->n_holders() == 1);
}

// many threads join, read, try to mutate, build the late piece and leave, while the donor leaves in the middle
static void threads(int n_threads, int rounds) {
    for (int r = 0; r < rounds; ++r) {
        const int freed0 = FakeSet::freed.load();
        auto set = fresh(true);
        std::unique_ptr<SetHold<FakeSet>> donor(new SetHold<FakeSet>(set));
        set.reset();
        std::atomic<int> builds{0}, refused{0}, go{0};
        std::vector<std::unique_ptr<SetHold<FakeSet>>> first;
        for (int i = 0; i < n_threads; ++i) first.push_back(share(donor->set));   // taken before the donor may leave
        std::vector<std::thread> th;
        for (int i = 0; i < n_threads; ++i)
            th.emplace_back([&, i] {
                std::unique_ptr<SetHold<FakeSet>> mine = std::move(first[(size_t)i]);
                while (!go.load()) std::this_thread::yield();
                FakeSet& s = *mine->set;
                if (s.build_once([&] { return s.table != nullptr; }, [&]() -> int64_t { s.table = new int[64](); s.table[3] = 11; return 256; })) builds.fetch_add(1);
                if (!s.mutation_refusal().empty()) refused.fetch_add(1);
                (void)s.finalize_is_noop();
                auto more = share(mine->set);                        // a sharer of a sharer
                if (more) { CHECK(more->set->table && more->set->table[3] == 11); CHECK(more->set->payload->at(9) == 7); }
                CHECK(s.n_bytes() == 4096 + 256);
                more.reset();
                mine.reset();
            });
        go.store(1);
        donor.reset();                                               // while the others run
        for (auto& t : th) t.join();
        CHECK(builds.load() == 1);
        CHECK(FakeSet::live.load() == 0 && FakeSet::freed.load() == freed0 + 1);
        (void)refused;
    }
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    rules();
    throwing_holder();
    threads(8, rounds);
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("weight_share_sanitize: ok (%d threaded rounds)\n", rounds);
    return 0;
}
