// Host-side check of the merge / subset copy of IVF-PQ codes (csrc/k_merge.h) — built and run by tests/test_merge_layout_host.py (no GPU
// needed).  The append is emulated on host memory with the very functions the kernel runs (mg_push_items -> work items, then per thread
// of an item mg_pq_byte, and mg_pq_run wherever the 16-byte form applies), for every ordered pair of code layouts that applies at M = 16, 24, 64, 96, destination lengths 0 .. 600 (crossing
// the 16 / 32 / 64-row blocks and the 512-row sliced group) and source counts {0, 1, 15, 33, 513}, from a source run that starts at a
// varying phase of its own blocks (and, for part of the cases, from a scattered row selection):
//   * every (row, m) byte of the source run arrives at (destination row, m) of the destination layout;
//   * the padding bytes m in [M, Mpad) arrive as zero whatever the source held there;
//   * nothing else is written (the rest of the destination buffer keeps its sentinel);
//   * offsets formed from rows beyond 2^32 bytes do not truncate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../../retrieval-scaling_amd/csrc/k_merge.h"

using namespace rsx;

static inline uint8_t code_of(int64_t row, int m) { return (uint8_t)(1 + ((row * 131 + m * 17 + (row >> 7)) % 254)); }      // never 0, never the sentinel

struct Layout { int M, Mpad, CB; const char* name; };

// form 0: byte by byte (mg_pq_byte); form 1: the 16-byte runs (mg_pq_run), where both layouts keep them together
static int run_pair(const Layout& S, const Layout& D, int form, long long& ncases) {
    const int M = S.M, Mpad = S.Mpad;
    const uint8_t SENT = 0xFF;
    const int64_t srows = 2560, drows = 1536, sbase = 512;
    std::vector<uint8_t> src((size_t)(srows * Mpad)), dst((size_t)(drows * Mpad), SENT), clean((size_t)(drows * Mpad), SENT);
    for (int64_t r = 0; r < srows; r++)
        for (int m = 0; m < Mpad; m++) src[(size_t)pq_code_addr(r, m, Mpad, S.CB)] = m < M ? code_of(r, m) : (uint8_t)0xEE;      // garbage in the source's padding
    std::vector<uint32_t> sel_rows;
    std::vector<MergeItem> items;
    const int counts[] = {0, 1, 15, 33, 513};
    for (int64_t dlen = 0; dlen <= 600; dlen++)
        for (int cnt : counts)
            for (int sel = 0; sel < (dlen % 5 == 0 ? 2 : 1); sel++) {
                ncases++;
                const int64_t first = (dlen * 7 + cnt) % 67;      // phase of the source run inside its blocks
                items.clear(); sel_rows.clear();
                if (sel) {
                    // a scattered selection in list order: gaps of 1 .. 3 rows; the items index sel_rows from a non-zero offset
                    sel_rows.assign(5, 0xDEADBEEFu);
                    int64_t r = sbase + first;
                    for (int j = 0; j < cnt; j++) { sel_rows.push_back((uint32_t)r); r += 1 + (j * 5 + dlen) % 3; }
                    if (r > srows) { std::printf("FAIL the check's own source buffer is too small\n"); return 1; }
                    mg_push_items(items, 5, dlen, cnt, 1);
                } else {
                    mg_push_items(items, sbase + first, dlen, cnt, 0);
                }
                int64_t covered = 0;
                for (const MergeItem& it : items) {
                    if (it.n <= 0 || it.n > MG_TILE || it.dst != dlen + covered) { std::printf("FAIL work items do not tile the run (%s -> %s)\n", S.name, D.name); return 1; }
                    covered += it.n;
                    if (form == 0)
                        for (int64_t t = 0; t < (int64_t)it.n * Mpad; t++) mg_pq_byte(it, t, sel_rows.data(), src.data(), dst.data(), M, Mpad, S.CB, D.CB);
                    else
                        for (int64_t t = 0; t < (int64_t)it.n * (Mpad >> 4); t++) mg_pq_run(it, t, sel_rows.data(), src.data(), dst.data(), M, Mpad, S.CB, D.CB);
                }
                if (covered != cnt) { std::printf("FAIL work items cover %lld of %d rows\n", (long long)covered, cnt); return 1; }
                // every byte arrived (and is put back to the sentinel), then nothing else may differ from the sentinel
                for (int j = 0; j < cnt; j++) {
                    const int64_t srow = sel ? (int64_t)sel_rows[(size_t)(5 + j)] : sbase + first + j;
                    for (int m = 0; m < Mpad; m++) {
                        uint8_t& b = dst[(size_t)pq_code_addr(dlen + j, m, Mpad, D.CB)];
                        const uint8_t want = m < M ? code_of(srow, m) : (uint8_t)0;
                        if (b != want) {
                            std::printf("FAIL %s -> %s M=%d form %d dlen=%lld cnt=%d sel=%d: row %d m %d holds %d, expected %d\n", S.name, D.name, M, form, (long long)dlen, cnt, sel, j,
                                        m, (int)b, (int)want);
                            return 1;
                        }
                        b = SENT;
                    }
                }
                if (memcmp(dst.data(), clean.data(), dst.size()) != 0) {
                    std::printf("FAIL %s -> %s M=%d dlen=%lld cnt=%d sel=%d: a byte outside the appended rows was written\n", S.name, D.name, M, (long long)dlen, cnt, sel);
                    return 1;
                }
            }
    return 0;
}

int main() {
    const Layout all[] = {{16, 16, 16, "granule16"}, {16, 16, 0, "rotated"}, {24, 24, 4, "granule4"}, {64, 64, 16, "granule16"}, {64, 64, 0, "rotated"},
                          {96, 96, 16, "granule16"}, {96, 96, 0, "rotated"}, {96, 96, PQ_SLICED, "sliced"},
                          {12, 16, 16, "granule16 (M = 12 of 16)"}};      // (beside the four M of the pairs: padding inside a 16-byte run)
    // one host thread per ordered pair of layouts
    struct Job { const Layout *S, *D; int form; long long ncases = 0; int rc = 0; };
    std::vector<Job> jobs;
    int npairs = 0, nrunpairs = 0;
    for (const Layout& S : all)
        for (const Layout& D : all) {
            if (S.M != D.M) continue;
            npairs++;
            jobs.push_back(Job{&S, &D, 0});
            if (mg_pq_runs_apply(S.CB, D.CB)) { nrunpairs++; jobs.push_back(Job{&S, &D, 1}); }
        }
    std::vector<std::thread> th;
    for (Job& j : jobs) th.emplace_back([&j] { j.rc = run_pair(*j.S, *j.D, j.form, j.ncases); });
    for (std::thread& t : th) t.join();
    long long ncases = 0;
    for (const Job& j : jobs) { if (j.rc) return 1; ncases += j.ncases; }
    if (nrunpairs != npairs - 1) { std::printf("FAIL the 16-byte form must serve every pair but the 4-byte granule's\n"); return 1; }
    // 64-bit offsets: a row 2^33 rows further on lies exactly 2^33 * Mpad bytes further on, in every layout; row strides likewise
    for (const Layout& L : all) {
        const int64_t far = (int64_t)1 << 33;      // a multiple of every block, slab and group size
        for (int64_t r : {(int64_t)0, (int64_t)17, (int64_t)63, (int64_t)511, (int64_t)777})
            for (int m = 0; m < L.Mpad; m += 5)
                if (pq_code_addr(far + r, m, L.Mpad, L.CB) - pq_code_addr(r, m, L.Mpad, L.CB) != far * L.Mpad) {
                    std::printf("FAIL 64-bit offset %s M=%d row %lld m %d\n", L.name, L.M, (long long)r, m);
                    return 1;
                }
    }
    if (mg_row_off(3000000000ll, 3072) != 9216000000000ll || mg_row_off(((int64_t)1 << 32) + 5, 768) != (((int64_t)1 << 32) + 5) * 768) {
        std::printf("FAIL 64-bit row offset\n");
        return 1;
    }
    {
        const uint32_t rows[2] = {0xFFFFFFF0u, 7u};
        const MergeItem a{((int64_t)1 << 33) + 3, 0, 2, 0}, b{0, 0, 2, 1};
        if (mg_src_row(a, 1, nullptr) != ((int64_t)1 << 33) + 4 || mg_src_row(b, 0, rows) != 0xFFFFFFF0ll) { std::printf("FAIL 64-bit source row\n"); return 1; }
    }
    // the subset predicates
    if (!mg_id_selected(MG_SUBSET_ID_RANGE, 5, 5, 6) || mg_id_selected(MG_SUBSET_ID_RANGE, 6, 5, 6) || !mg_id_selected(MG_SUBSET_ID_MOD, 10, 3, 1) ||
        mg_id_selected(MG_SUBSET_ID_MOD, -2, 3, 1)) { std::printf("FAIL subset predicate\n"); return 1; }
    std::printf("merge ok: %d layout pairs, %lld cases\n", npairs, ncases);
    return 0;
}
