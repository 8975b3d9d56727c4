// Host-only check of speq_amd/csrc/scan_plan.hpp (tests/test_scan_plan_cpu.py compiles this with plain g++ and no ROCm
// include path: that it compiles is the proof that the header needs no HIP).
//   line 1 of the output: the packed value of every variant for which compiled() holds
//   then, per line of facts on stdin (the fields of ScanFacts in declaration order, as integers):
//   "<packed variant> <last_kernel> <grid> <buf_bytes> <lds_bytes> <lds_launch> <table_read>"
#include <cstdio>

#include "scan_plan.hpp"

int main() {
    for (int x = 0; x < (1 << 14); ++x)
        if (speq::compiled(speq::ScanVariant::unpack(x))) std::printf("%d ", x);
    std::printf("\n");
    long long in[24];
    for (;;) {
        for (long long& x : in)
            if (std::scanf("%lld", &x) != 1) return 0;
        speq::ScanFacts f;
        int i = 0;
        f.mode = (int)in[i++], f.paired = in[i++] != 0, f.em = in[i++] != 0, f.stats = in[i++] != 0;
        f.k = (uint32_t)in[i++], f.G = (uint32_t)in[i++], f.units = (uint64_t)in[i++];
        f.ilp = (uint32_t)in[i++], f.ilp_local = (uint32_t)in[i++], f.ilp_kt = (uint32_t)in[i++];
        f.kt_pipeline = in[i++] != 0;
        f.blocks_per_cu = (uint32_t)in[i++], f.blocks_per_cu_kt = (uint32_t)in[i++], f.blocks_per_cu_ax = (uint32_t)in[i++];
        f.grid_blocks = (uint32_t)in[i++], f.grid_blocks_kt = (uint32_t)in[i++], f.grid_blocks_ax = (uint32_t)in[i++];
        f.ax_generations = (uint32_t)in[i++], f.n_cus = (uint32_t)in[i++];
        f.ax_usable = in[i++] != 0, f.sproof_active = in[i++] != 0, f.table = (int)in[i++];
        f.ax_wpb = (uint32_t)in[i++], f.ax_wave_bytes = (uint32_t)in[i++];
        const speq::ScanPlan p = speq::plan_scan(f);
        std::printf("%d %d %u %u %zu %zu %d\n", p.variant.pack(), p.last_kernel, p.grid, p.buf_bytes, p.lds_bytes,
                    p.lds_launch, (int)p.table_read);
    }
}
