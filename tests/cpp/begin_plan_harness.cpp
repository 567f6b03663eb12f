// Command interpreter over q3_begin_plan.h for tests/test_cpu_begin_plan.py: one command per line on stdin, one answer per line on stdout.
//   limits B MAX_CTX MAX_TRAILING MAX_FRAMES_CAP ROWS_MAX MFMA_MIN_ROWS MFMA_DIMS          -> ok
//   plan ENTRY MAX_NEW N { SLOT S N_TRAILING N_PREFIX MAX_FRAMES KV_TOKENS P FLAGS } x N   ENTRY: 0 plain, 1 prefixed, 2 ragged
//       FLAGS: 1 prompt given, 2 trailing given, 4 codes given, 8 the codes hold a bad id, 16 the prefix id is unknown; P: what the id resolves to
//       -> err TEXT | ok m TOKENS,CAP,ARMED_MAX_FRAMES,POS ... [forced | g I0,G,BATCHED,CONSECUTIVE ... | rows TOTAL]
//       what the entry does with the plan, in the entry's order: the member checks; plain then hands a lone member with forced frames to
//       the forced begin, and otherwise walks its groups with its own look for a slot listed twice; prefixed walks its groups; ragged
//       counts the rows it stages
//   ragged TOTAL SEG_KERNELS SEAM_STEP                                                      -> one_at_a_time 0|1
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "q3_begin_plan.h"

int main() {
    q3::BeginLimits L;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        try {
            if (cmd == "limits") {
                int dims = 0;
                in >> L.B >> L.max_ctx >> L.max_trailing >> L.max_frames_cap >> L.rows_max >> L.mfma_min_rows >> dims;
                L.mfma_dims = dims != 0;
                std::cout << "ok\n";
            } else if (cmd == "plan") {
                int e = 0, max_new = 0, n = 0;
                in >> e >> max_new >> n;
                std::vector<q3::BeginMember> m((size_t)n);
                std::vector<int> P((size_t)n), flags((size_t)n);
                for (int i = 0; i < n; ++i) {
                    q3::BeginMember& q = m[(size_t)i];
                    in >> q.slot >> q.S >> q.n_trailing >> q.n_prefix >> q.max_frames >> q.kv_tokens >> P[(size_t)i] >> flags[(size_t)i];
                    q.has_prompt = flags[(size_t)i] & 1; q.has_trailing = flags[(size_t)i] & 2; q.has_codes = flags[(size_t)i] & 4;
                }
                if (!in) throw std::runtime_error("harness: short plan line");
                const q3::BeginEntry entry = (q3::BeginEntry)e;
                q3::begin_check<std::runtime_error>(entry, m.data(), n, max_new, L,
                    [&](int i) { if (flags[(size_t)i] & 16) throw std::runtime_error("unknown prefix id"); return P[(size_t)i]; },
                    [&](int i) { if (flags[(size_t)i] & 8) throw std::runtime_error("frame codes: bad id"); });
                std::ostringstream out;
                out << "ok m";
                for (const q3::BeginMember& q : m)
                    out << " " << q3::begin_tokens(q, max_new) << "," << q3::begin_cap(q, max_new) << "," << q3::begin_armed_max_frames(q, max_new) << "," << q3::begin_own(q);
                if (entry == q3::BEGIN_RAGGED) out << " rows " << q3::begin_ragged_rows(m.data(), n);
                else if (entry == q3::BEGIN_PLAIN && n == 1 && m[0].n_prefix > 0) out << " forced";
                else {
                    out << " g";
                    for (const q3::BeginGroup& gr : q3::begin_groups(entry, m.data(), n, L)) {
                        if (entry == q3::BEGIN_PLAIN) q3::begin_check_group_slots<std::runtime_error>(m.data(), gr);
                        out << " " << gr.i0 << "," << gr.g << "," << gr.batched << "," << gr.consecutive;
                    }
                }
                std::cout << out.str() << "\n";
            } else if (cmd == "ragged") {
                size_t total = 0;
                int seg = 0, seam = 0;
                in >> total >> seg >> seam;
                std::cout << "one_at_a_time " << q3::begin_ragged_one_at_a_time(total, L, seg != 0, seam != 0) << "\n";
            } else std::cout << "err unknown command\n";
        } catch (const std::exception& ex) { std::cout << "err " << ex.what() << "\n"; }
    }
    return 0;
}
