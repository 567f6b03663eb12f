#!/bin/bash
# AddressSanitizer + UBSan, then ThreadSanitizer, over the host-only bookkeeping of a shared weight set (csrc/q3_weight_share.h); CPU only.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
D=$(mktemp -d)
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -I "$ROOT/leaxer-qwen3-tts_amd/csrc" \
    "$ROOT/tools/weight_share_sanitize.cpp" -o "$D/ws_asan"
"$D/ws_asan" "${1:-200}"
g++ -std=c++17 -O1 -g -pthread -fsanitize=thread -I "$ROOT/leaxer-qwen3-tts_amd/csrc" "$ROOT/tools/weight_share_sanitize.cpp" -o "$D/ws_tsan"
"$D/ws_tsan" "${1:-200}"
rm -rf "$D"
