// Command interpreter over q3_codec_plan.h for tests/test_cpu_codec_plan.py: one command per line on stdin, one answer per line on stdout.
//   cfg CODEBOOK HIDDEN HEADS HEAD_DIM FFN TRIM N_UP RATIO x N_UP N_BLOCKS RATE x N_BLOCKS      -> ok
//   ctx                                  -> codec_stage_b_context
//   len F                                -> codec_decode_len (the raw formula) and codec_len_of (0 for F <= 0)
//   up                                   -> rows per frame behind the ConvNeXt stages, samples per frame
//   cut A0 N CTX N_WIN FILLS             -> FIRST N_OWN MATCHES
//   groups CTXB G { N_DONE N } x G       -> o INDEX ... g I0,I1,TW ...      the batched push's order (indices into the call) and its groups
//   bytes batch N FP P UPSAMPLING | stream T | push T BACK_ROWS | prime G FP PS                 -> the arena's bytes
//   bump NFLOAT ...                      -> the offsets a planning CodecBump hands out, then its total
//   codes N V x N                        -> err TEXT | ok V ...               stage_codes against the codebook
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "q3_codec_plan.h"

int main() {
    q3tts_config c{};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        try {
            if (cmd == "cfg") {
                c = q3tts_config{};
                in >> c.cd_codebook >> c.cd_hidden >> c.cd_heads >> c.cd_head_dim >> c.cd_ffn >> c.cd_tconv_trim >> c.cd_n_up;
                if (!in || c.cd_n_up < 0 || c.cd_n_up > 4) throw std::runtime_error("harness: bad cfg line");
                for (int i = 0; i < c.cd_n_up; ++i) in >> c.cd_up_ratios[i];
                in >> c.cd_n_blocks;
                if (!in || c.cd_n_blocks < 0 || c.cd_n_blocks > 8) throw std::runtime_error("harness: bad cfg line");
                for (int i = 0; i < c.cd_n_blocks; ++i) in >> c.cd_up_rates[i];
                if (!in) throw std::runtime_error("harness: short cfg line");
                std::cout << "ok\n";
            } else if (cmd == "ctx") {
                std::cout << q3::codec_stage_b_context(c) << "\n";
            } else if (cmd == "len") {
                int F = 0;
                in >> F;
                std::cout << q3::codec_decode_len(c, F) << " " << q3::codec_len_of(c, F) << "\n";
            } else if (cmd == "up") {
                std::cout << q3::codec_up_front(c) << " " << q3::codec_samples_per_frame(c) << "\n";
            } else if (cmd == "cut") {
                int a0 = 0, n = 0, ctx = 0, fills = 0;
                int64_t n_win = 0;
                in >> a0 >> n >> ctx >> n_win >> fills;
                const q3::CodecCut k = q3::codec_window_cut(c, a0, n, ctx);
                std::cout << k.first << " " << k.n_own << " " << k.matches(n_win, fills != 0) << "\n";
            } else if (cmd == "groups") {
                int ctxB = 0, g = 0;
                in >> ctxB >> g;
                if (!in || g < 0) throw std::runtime_error("harness: bad groups line");
                std::vector<int> n_done((size_t)g), n((size_t)g), live;
                for (int i = 0; i < g; ++i) { in >> n_done[(size_t)i] >> n[(size_t)i]; live.push_back(i); }
                if (!in) throw std::runtime_error("harness: short groups line");
                auto left = [&](int x) { return std::min(n_done[(size_t)x], ctxB); };
                q3::codec_push_order(live, left);
                std::ostringstream out;
                out << "o";
                for (int x : live) out << " " << x;
                out << " g";
                for (const q3::CodecGroup& G : q3::codec_push_groups(g, [&](int i) { return left(live[(size_t)i]); }, [&](int i) { return n[(size_t)live[(size_t)i]]; }))
                    out << " " << G.i0 << "," << G.i1 << "," << G.Tw;
                std::cout << out.str() << "\n";
            } else if (cmd == "bytes") {
                std::string kind;
                size_t a = 0, b = 0, d = 0, e = 0;
                in >> kind >> a >> b >> d >> e;   // the kinds with fewer numbers leave the rest 0
                if (kind == "batch") std::cout << q3::codec_batch_arena_bytes(c, a, b, d, e != 0) << "\n";
                else if (kind == "stream") std::cout << q3::codec_stream_arena_bytes(c, a) << "\n";
                else if (kind == "push") std::cout << q3::codec_sbatch_push_bytes(c, a, b) << "\n";
                else if (kind == "prime") std::cout << q3::codec_sbatch_prime_bytes(c, a, b, d) << "\n";
                else throw std::runtime_error("harness: unknown arena");
            } else if (cmd == "bump") {
                q3::CodecBump take;
                std::ostringstream out;
                size_t nfloat = 0;
                while (in >> nfloat) { const size_t at = take.off; if (take(nfloat) != nullptr) throw std::runtime_error("harness: a planning bump returned memory"); out << at << " "; }
                std::cout << out.str() << take.off << "\n";
            } else if (cmd == "codes") {
                size_t n = 0;
                in >> n;
                std::vector<int64_t> v(n);
                for (size_t i = 0; i < n; ++i) in >> v[i];
                if (!in) throw std::runtime_error("harness: short codes line");
                std::vector<int32_t> dst(n, -7);
                q3::stage_codes<std::runtime_error>(v.data(), n, c.cd_codebook, dst.data());
                std::ostringstream out;
                out << "ok";
                for (int32_t x : dst) out << " " << x;
                std::cout << out.str() << "\n";
            } else std::cout << "err unknown command\n";
        } catch (const std::exception& ex) { std::cout << "err " << ex.what() << "\n"; }
    }
    return 0;
}
