// Host-only check of the row quantisers' launch ladder (fp8-mps-metal_amd/csrc/fp8mi_rowquant.h: row_rung) against its thresholds
// written out as a table.  Built and run by tests/test_abi_and_host.py (the host half of a HIP compile: no GPU, no libfp8mi.so).
#include <cstdio>

#include "../../fp8-mps-metal_amd/csrc/fp8mi_rowquant.h"

namespace {

struct Expect {
    int w, nv;
};

// pieces: 16-byte pieces per lane of ONE wave that holds the row
Expect expected(long cols, int kPer, bool is_f32, bool rowwise)
{
    const long pieces = (cols / kPer + 63) / 64;
    if (cols > 16384) return {0, 0};                 // looping
    if (rowwise && pieces <= 2) return {1, 2};       // the rowwise quantiser's NV = 2 rung
    if (pieces <= 8) return {1, 8};
    if (pieces <= 32) return {4, 8};
    if (is_f32 && pieces <= 64) return {8, 8};
    return {0, 0};                                   // looping
}

}  // namespace

int main()
{
    int bad = 0;
    for (int kPer : {4, 8}) {
        for (int is_f32 = 0; is_f32 < 2; ++is_f32) {
            for (int rowwise = 0; rowwise < 2; ++rowwise) {
                for (long cols = 0; cols <= 20000; ++cols) {
                    const Expect e = expected(cols, kPer, is_f32 != 0, rowwise != 0);
                    const RowRung g = row_rung(cols, kPer, is_f32 != 0, rowwise != 0);
                    if ((g.w != e.w || g.nv != e.nv) && bad++ < 10)
                        std::printf("cols=%ld kPer=%d f32=%d rowwise=%d: rung (%d, %d), expected (%d, %d)\n", cols, kPer, is_f32, rowwise, g.w, g.nv, e.w,
                                    e.nv);
                }
            }
        }
    }
    // the edges by their numbers: 16-bit input (kPer 8) and fp32 input (kPer 4)
    const struct {
        long cols;
        int kPer, f32, rowwise, w, nv;
    } edges[] = {{0, 8, 0, 0, 1, 8},     {4096, 8, 0, 0, 1, 8},  {4103, 8, 0, 0, 1, 8},  {4104, 8, 0, 0, 4, 8},  {16384, 8, 0, 0, 4, 8}, {16385, 8, 0, 0, 0, 0},
                 {1024, 8, 0, 1, 1, 2},  {1031, 8, 0, 1, 1, 2},  {1032, 8, 0, 1, 1, 8},  {2048, 4, 1, 0, 1, 8},  {2052, 4, 1, 0, 4, 8},  {8192, 4, 1, 0, 4, 8},
                 {8195, 4, 1, 0, 4, 8},  {8196, 4, 1, 0, 8, 8},  {16384, 4, 1, 0, 8, 8}, {16385, 4, 1, 0, 0, 0}, {8196, 4, 0, 0, 0, 0},  {512, 4, 1, 1, 1, 2},
                 {516, 4, 1, 1, 1, 8},    {2048, 8, 0, 0, 1, 8},  {2048, 8, 0, 1, 1, 8},  {1024, 8, 0, 0, 1, 8},  {1031, 8, 0, 0, 1, 8},  {512, 4, 1, 0, 1, 8},
                 {0, 8, 0, 1, 1, 2},     {16384, 8, 0, 1, 4, 8}, {16385, 8, 0, 1, 0, 0}, {4104, 8, 0, 1, 4, 8}};
    for (const auto &e : edges) {
        const RowRung g = row_rung(e.cols, e.kPer, e.f32 != 0, e.rowwise != 0);
        if ((g.w != e.w || g.nv != e.nv) && bad++ < 20)
            std::printf("edge cols=%ld kPer=%d f32=%d rowwise=%d: rung (%d, %d), expected (%d, %d)\n", e.cols, e.kPer, e.f32, e.rowwise, g.w, g.nv, e.w, e.nv);
    }
    std::printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
