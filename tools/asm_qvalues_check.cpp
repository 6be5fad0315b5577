// asm_qvalues_check -- hm_asm_qvalues (host only) over the inputs of tests/test_pileup_asm_q_cpu.py, as a stand-alone program
// that host sanitizers can watch.  `python tests/asm_q_ref.py cases.bin` writes the cases with the q-values numpy gives;
// this program solves each case and compares bit for bit, then feeds one refusal.  Built with the engine's source, e.g.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++20 -Xarch_host -fsanitize=address,undefined \
//         hifimeth_amd/csrc/hm_pileup.hip tools/asm_qvalues_check.cpp -o asm_qvalues_check && ./asm_qvalues_check cases.bin
// No device is touched: it runs on a machine without a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/hifimeth_hip.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "USAGE: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    static_assert(sizeof(hm_asm_bin_t) == 32 && sizeof(hm_asm_t) == 48 && sizeof(hm_asmq_t) == 56, "struct sizes");
    int n_cases = 0, bad = 0;
    int64_t n[2];
    while (fread(n, sizeof n, 1, f) == 1) {
        std::vector<hm_asm_bin_t> tab;
        std::vector<hm_asm_t> big;
        std::vector<double> want_tq, want_bq;
        std::vector<uint64_t> want_m;
        if (!read_n(f, tab, (size_t)n[0]) || !read_n(f, big, (size_t)n[1]) || !read_n(f, want_tq, (size_t)n[0]) ||
            !read_n(f, want_bq, (size_t)n[1]) || !read_n(f, want_m, 3)) { fprintf(stderr, "truncated case\n"); return 2; }
        std::vector<double> big_q((size_t)n[1]);
        uint64_t m[3];
        // exact-size heap blocks, no spare element: a read or write past either end is the sanitizer's to report
        const int rc = hm_asm_qvalues(tab.data(), n[0], big.data(), n[1], big_q.data(), m);
        bool ok = rc == HM_OK && memcmp(m, want_m.data(), sizeof m) == 0;
        for (size_t i = 0; ok && i < tab.size(); ++i) ok = memcmp(&tab[i].qvalue, &want_tq[i], 8) == 0;
        for (size_t i = 0; ok && i < big.size(); ++i) ok = memcmp(&big_q[i], &want_bq[i], 8) == 0;
        printf("case %d: %lld bins, %lld big loci: %s\n", n_cases, (long long)n[0], (long long)n[1], ok ? "ok" : "MISMATCH");
        bad += !ok;
        ++n_cases;
        if (tab.size() > 1) {  // a refusal: descending bins, outputs untouched
            std::swap(tab[0], tab[1]);
            const double before = tab[0].qvalue;
            uint64_t m2[3] = {9, 9, 9};
            if (hm_asm_qvalues(tab.data(), n[0], big.data(), n[1], big_q.data(), m2) != HM_EINVAL || m2[0] != 9 ||
                memcmp(&tab[0].qvalue, &before, 8) != 0) { printf("  refusal: MISMATCH\n"); ++bad; }
        }
    }
    fclose(f);
    printf("%d cases, %d bad\n", n_cases, bad);
    return bad || !n_cases ? 1 : 0;
}
