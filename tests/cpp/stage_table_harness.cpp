// Command interpreter over q3_stage.h for tests/test_cpu_stage_table.py: one command per line on stdin, one answer per line on stdout.
// The stage is a toy with the shape of the real ones: a slot has a look-ahead `delay`, its rule emits max(0, received - delay) samples
// while it runs and everything once it is finished, and its commit flips the carry when the push leaves one (not finished).
//   init MAX | begin DELAY | end ID | get ID | len ID N FINISH | push ID N FINISH | state ID
#include <algorithm>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

#include "q3_stage.h"

struct ToySlot : q3::StageSlot { int64_t delay = 0; };
using Table = q3::StageTable<ToySlot, std::runtime_error>;

static int64_t rule(const ToySlot& S, int64_t n, bool finish) { return finish ? n : std::max<int64_t>(0, n - S.delay); }

int main() {
    Table tab{ "pcm sink", "sink", "no such sink", 0, {} };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        long long a = 0, b = 0, c = 0;
        in >> cmd >> a >> b >> c;
        try {
            if (cmd == "init") { tab.max = (int)a; tab.slots.clear(); std::cout << "ok\n"; }
            else if (cmd == "begin") { const int id = tab.free_id(); tab.open(id).delay = a; std::cout << "id " << id << "\n"; }
            else if (cmd == "end") { tab.end((int)a); std::cout << "ok\n"; }
            else if (cmd == "get") { const int64_t d = tab.get((int)a).delay; std::cout << "delay " << d << "\n"; }
            else if (cmd == "len") { const int64_t n = tab.push_len((int)a, b, c != 0, rule); std::cout << "len " << n << "\n"; }
            else if (cmd == "push") {   // what a stage's launch + commit do to the table
                const int64_t n_out = tab.push_len((int)a, b, c != 0, rule);
                tab.commit((int)a, b, n_out, c != 0, c == 0 && b > 0);
                std::cout << "out " << n_out << "\n";
            }
            else if (cmd == "state") {   // no check of the id: ended entries are inspected too
                const ToySlot& S = tab.slots.at((size_t)a);
                std::cout << "state used " << S.used << " finished " << S.finished << " cur " << S.cur << " n_in " << S.n_in << " n_out " << S.n_out << "\n";
            }
            else std::cout << "err unknown command\n";
        } catch (const std::exception& ex) { std::cout << "err " << ex.what() << "\n"; }
    }
    return 0;
}
