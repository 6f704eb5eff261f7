// Host-side check of the direct map's hash table (csrc/rsx_reconstruct.h: dm_hash_slot / dm_hash_next / dm_hash_find / dm_hash_insert_seq) —
// built with the host sanitizers and run by tests/test_reconstruct_host.py (no GPU needed, no kernel launch).  The table is what
// k_dm_hash_build fills with atomics and k_reconstruct probes; here one thread inserts and looks up through the same functions:
//   sequential ids, strided ids, ids that collide modulo the capacity, an id stored twice (the lowest row wins), absent ids (not found,
//   and the probe stops at a free slot long before it has gone round the table).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../retrieval-scaling_amd/csrc/rsx_reconstruct.h"

using namespace rsx;

struct Table {
    uint64_t cap, mask;
    std::vector<unsigned long long> w;
    explicit Table(int64_t n) : cap(dm_hash_capacity(n)), mask(cap - 1), w(2 * cap) {
        for (uint64_t s = 0; s < cap; s++) { w[2 * s] = DM_EMPTY; w[2 * s + 1] = DM_NO_ROW; }
    }
    bool insert(int64_t id, unsigned long long row) { return dm_hash_insert_seq(w.data(), mask, id, row); }
    unsigned long long find(int64_t id, int* steps = nullptr) const { return dm_hash_find(w.data(), mask, id, steps); }
};

static int fail(const char* what, long long a, long long b) { std::printf("FAIL %s (%lld, %lld)\n", what, a, b); return 1; }

// insert ids[i] -> row i, then every id is found at its row and `absent` ids are not found, with bounded probes
static int round_trip(const char* what, const std::vector<int64_t>& ids, const std::vector<int64_t>& absent, int max_steps) {
    Table t((int64_t)ids.size());
    if (t.cap < 2 * ids.size() || (t.cap & t.mask) != 0 || (t.cap > 2 && t.cap >= 4 * ids.size())) return fail("capacity is not the power of two >= 2 n", (long long)t.cap, (long long)ids.size());
    for (size_t i = 0; i < ids.size(); i++) if (!t.insert(ids[i], i)) return fail(what, (long long)i, -1);
    int worst = 0;
    for (size_t i = 0; i < ids.size(); i++) {
        int steps = 0;
        if (t.find(ids[i], &steps) != i) return fail(what, (long long)ids[i], (long long)i);
        if (steps > worst) worst = steps;
    }
    for (int64_t a : absent) {
        int steps = 0;
        if (t.find(a, &steps) != DM_NO_ROW) return fail("an absent id was found", (long long)a, 0);
        if (steps > worst) worst = steps;
    }
    if (worst > max_steps) return fail("probe length", worst, max_steps);
    std::printf("%s: n %zu, capacity %llu, longest probe %d\n", what, ids.size(), (unsigned long long)t.cap, worst);
    return 0;
}

int main() {
    const int64_t n = 6000;
    std::vector<int64_t> seq, strided, big, absent;
    for (int64_t i = 0; i < n; i++) { seq.push_back(i); strided.push_back(7 * i + 1000003); big.push_back(((int64_t)1 << 33) + 3 * i); }
    for (int64_t i = 0; i < 2000; i++) { absent.push_back(n + i); absent.push_back(-1 - i); absent.push_back(((int64_t)1 << 40) + 977 * i); }
    // a mixing hash at load <= 1/2: probes stay short (the bound is generous; a broken probe sequence walks thousands of slots)
    if (round_trip("sequential", seq, absent, 64)) return 1;
    if (round_trip("strided", strided, absent, 64)) return 1;
    if (round_trip("above 2^32", big, absent, 64)) return 1;

    // ids that collide modulo the capacity: ids whose hash lands on ONE slot (found by search) chain through linear probing
    {
        const int64_t m = 40;
        Table t(m);
        std::vector<int64_t> coll;
        for (int64_t id = 0; (int64_t)coll.size() < m && id < 100000000; id++) if (dm_hash_slot(id, t.mask) == 5) coll.push_back(id);
        if ((int64_t)coll.size() != m) return fail("could not find colliding ids", (long long)coll.size(), m);
        for (int64_t i = 0; i < m; i++) if (!t.insert(coll[(size_t)i], (unsigned long long)(100 + i))) return fail("colliding insert", i, 0);
        for (int64_t i = 0; i < m; i++) {
            int steps = 0;
            if (t.find(coll[(size_t)i], &steps) != (unsigned long long)(100 + i)) return fail("colliding lookup", coll[(size_t)i], i);
            if (steps != i + 1) return fail("the i-th colliding id sits i slots behind the shared one", steps, i + 1);
            if (t.w[2 * ((5 + i) & t.mask)] != (unsigned long long)coll[(size_t)i]) return fail("linear probing order", i, 0);
        }
        // an absent id of the same slot walks the whole chain and stops at the free slot behind it
        int64_t extra = -1;
        for (int64_t id = coll.back() + 1; id < 200000000; id++) if (dm_hash_slot(id, t.mask) == 5) { extra = id; break; }
        int steps = 0;
        if (extra < 0 || t.find(extra, &steps) != DM_NO_ROW || steps != m + 1) return fail("absent id behind a chain", steps, m + 1);
        // a full table (never built by the library: load <= 1/2) still terminates
        Table full(1);
        full.insert(1, 0); full.insert(2, 1);
        if (full.insert(3, 2)) return fail("insert into a full table", 0, 0);
        if (full.find(3) != DM_NO_ROW) return fail("lookup in a full table", 0, 0);
        std::printf("collisions: chain of %lld at one slot ok\n", (long long)m);
    }
    // an id stored more than once keeps one slot; the lowest row wins, whatever the order of arrival
    {
        Table t(8);
        t.insert(42, 900); t.insert(7, 3); t.insert(42, 17); t.insert(42, 500); t.insert(-5, 1); t.insert(42, 18);
        if (t.find(42) != 17 || t.find(7) != 3 || t.find(-5) != 1) return fail("repeated id", (long long)t.find(42), 17);
        int used = 0;
        for (uint64_t s = 0; s < t.cap; s++) used += t.w[2 * s] != DM_EMPTY;
        if (used != 3) return fail("slots used by 3 distinct ids", used, 3);
        if (t.insert((int64_t)DM_EMPTY, 0) || t.find((int64_t)DM_EMPTY) != DM_NO_ROW) return fail("the free-slot word is not an id", 0, 0);
    }
    std::printf("direct map ok\n");
    return 0;
}
