// The claim discipline of the work-queue slot ring (bayhunter_amd/csrc/slot_ring.h, what SlotClaim of swd_launch.hip
// is built on) as a program of its own, no HIP: four threads take, use and give back the slots of a ring of 2 and of
// 8 with the mutex held where SlotClaim holds it.  A slot never has two holders (owner[] is written without the
// mutex, by the holder alone: a second holder is a data race under -fsanitize=thread and a failed check anywhere), a
// claim that leaves its scope without drop() frees its slot, and "all claimed" comes only when every slot is held.
// Built by tests/test_sanitizers.py with -fsanitize=address,undefined and with -fsanitize=thread.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "../../bayhunter_amd/csrc/slot_ring.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "slot_ring_sim: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {
std::mutex g_mutex;

int held_slots(const bh::SlotRing &r)           // with the mutex held
{
    int n = 0;
    for (int i = 0; i < bh::kQueueSlots; i++) n += r.claimed[i] ? 1 : 0;
    return n;
}

void one_thread(bh::SlotRing &ring, int *owner, int me, int rounds, long *refused)
{
    for (int k = 0; k < rounds; k++) {
        bh::RingClaim claim(g_mutex);
        {
            std::lock_guard<std::mutex> lock(g_mutex);
            if (claim.take(ring) < 0) {
                CHECK(held_slots(ring) == ring.nslots);
                ++*refused;
                continue;
            }
        }
        const int i = claim.index();
        CHECK(i >= 0 && i < ring.nslots && owner[i] == 0);
        owner[i] = me;
        std::this_thread::yield();
        CHECK(owner[i] == me);
        owner[i] = 0;
        if (k % 3 == 0) continue;               // no drop(): an early return after the claim
        std::lock_guard<std::mutex> lock(g_mutex);
        claim.drop();
    }
}

void run_ring(int nslots)
{
    bh::SlotRing ring;
    ring.nslots = nslots;
    int owner[bh::kQueueSlots] = {};
    long refused[4] = {};
    std::vector<std::thread> threads;
    for (int t = 0; t < 4; t++) threads.emplace_back(one_thread, std::ref(ring), owner, t + 1, 20000, &refused[t]);
    for (auto &t : threads) t.join();
    std::lock_guard<std::mutex> lock(g_mutex);
    CHECK(held_slots(ring) == 0);
    if (nslots >= 4) CHECK(refused[0] + refused[1] + refused[2] + refused[3] == 0);   // four threads, a slot each
    // one thread holds the whole ring: the next take is refused, and what is given back is what the one after it gets
    {
        std::vector<bh::RingClaim *> all;
        for (int i = 0; i < nslots; i++) {
            all.push_back(new bh::RingClaim(g_mutex));
            CHECK(all.back()->take(ring) >= 0);
        }
        bh::RingClaim late(g_mutex);
        CHECK(late.take(ring) == -1 && late.index() == -1 && held_slots(ring) == nslots);
        const int freed = all[nslots / 2]->index();
        all[nslots / 2]->drop();
        CHECK(late.take(ring) == freed && held_slots(ring) == nslots);
        late.drop();
        for (bh::RingClaim *c : all) { if (c->index() >= 0) c->drop(); delete c; }
    }
    CHECK(held_slots(ring) == 0);
}
}  // namespace

int main()
{
    run_ring(2);
    run_ring(8);
    {   // out of scope without drop(), no other thread about: the destructor takes the mutex itself
        bh::SlotRing ring;
        ring.nslots = 2;
        int first;
        {
            bh::RingClaim claim(g_mutex);
            std::lock_guard<std::mutex> lock(g_mutex);
            first = claim.take(ring);
        }
        std::lock_guard<std::mutex> lock(g_mutex);
        CHECK(first == 0 && held_slots(ring) == 0);
    }
    std::puts("slot ring ok");
    return 0;
}
