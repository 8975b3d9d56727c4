// Stand-alone driver of speq_amd/csrc/ax_decode.hpp for tests/test_ax_decode_cpu.py: includes nothing but that header
// and is compiled with plain g++ and no ROCm include path.
// stdin (binary, little-endian), any number of blocks: u32 n, u32 cutoff, then n records of 33 bytes: the chunk's 16
// base bytes, its 16 quality bytes, the quality byte before the chunk.
// stdout: per record four u32: the local-mode decode's code word and bad | change << 16, then the global-mode decode's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ax_decode.hpp"

int main() {
    uint32_t head[2];
    std::vector<unsigned char> in;
    std::vector<uint32_t> out;
    while (std::fread(head, 4, 2, stdin) == 2) {
        const uint32_t n = head[0], cutoff = head[1];
        in.resize((size_t)n * 33u);
        out.resize((size_t)n * 4u);
        if (std::fread(in.data(), 33, n, stdin) != n) return 2;
        const uint32_t qt4 = speq_dev::axd_qt4(cutoff), allbad = speq_dev::axd_allbad(cutoff);
        for (uint32_t r = 0; r < n; ++r) {
            const unsigned char* p = in.data() + (size_t)r * 33u;
            uint32_t sd[4], qd[4];
            for (int i = 0; i < 4; ++i) {
                sd[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
                        (uint32_t)p[4 * i + 3] << 24;
                qd[i] = (uint32_t)p[16 + 4 * i] | (uint32_t)p[16 + 4 * i + 1] << 8 | (uint32_t)p[16 + 4 * i + 2] << 16 |
                        (uint32_t)p[16 + 4 * i + 3] << 24;
            }
            uint32_t cw = 0, bad = 0, chb = 0;
            speq_dev::ax_decode_chunk<true>(sd, qd, qt4, allbad, p[32], cw, bad, chb);
            out[4u * r] = cw;
            out[4u * r + 1] = bad | chb << 16;
            speq_dev::ax_decode_chunk<false>(sd, qd, qt4, allbad, p[32], cw, bad, chb);
            out[4u * r + 2] = cw;
            out[4u * r + 3] = bad | chb << 16;
        }
        if (std::fwrite(out.data(), 16, n, stdout) != n) return 3;
    }
    return 0;
}
