// Host-only check of speq_amd/csrc/host_reads.hpp (tests/test_host_reads_cpu.py compiles this with plain g++ and no ROCm
// include path: that it compiles is the proof that the header needs no HIP).
//   per line of stdin "cut <step> <max_records> <max_bytes> <n> <len_0> ... <len_n-1>": the batch ends r1 of the reads
//   of those lengths, cut from r0 = 0 until r1 = n, on one line
//   per line "check <null_buffers> <n> <offset_0> ... <offset_n>": check_host_reads's message, or "ok"
//   per line "k <k>": check_report_k's message, or "ok"
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_reads.hpp"

int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        unsigned long long step = 0, max_records = 0, max_bytes = 0, n = 0, x = 0;
        try {
            if (!std::strcmp(what, "cut")) {
                if (std::scanf("%llu %llu %llu %llu", &step, &max_records, &max_bytes, &n) != 4) return 1;
                std::vector<uint64_t> off(n + 1, 0);
                for (uint64_t i = 0; i < n; ++i) {
                    if (std::scanf("%llu", &x) != 1) return 1;
                    off[i + 1] = off[i] + x;
                }
                for (uint64_t r0 = 0; r0 < n;) {
                    r0 = speq::next_batch(off.data(), n, r0, step, max_records, max_bytes);
                    std::printf("%llu ", (unsigned long long)r0);
                }
                std::printf("\n");
            } else if (!std::strcmp(what, "check")) {
                unsigned long long null_buffers = 0;
                if (std::scanf("%llu %llu", &null_buffers, &n) != 2) return 1;
                std::vector<uint64_t> off(n + 1, 0);
                for (uint64_t& o : off) {
                    if (std::scanf("%llu", &x) != 1) return 1;
                    o = x;
                }
                const std::vector<uint8_t> buf(off[n] + 1, 'A');
                const uint8_t* b = null_buffers ? nullptr : buf.data();
                speq::check_host_reads("who", b, b, off.data(), n);
                std::printf("ok\n");
            } else if (!std::strcmp(what, "k")) {
                if (std::scanf("%llu", &x) != 1) return 1;
                speq::check_report_k("who", (uint32_t)x);
                std::printf("ok\n");
            } else {
                return 1;
            }
        } catch (const std::invalid_argument& e) {
            std::printf("%s\n", e.what());
        }
    }
    return 0;
}
