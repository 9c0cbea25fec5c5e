// The host half of the resident servers' mailbox (csrc/evs_mailbox.h, included WITHOUT HIP) against a second thread that plays
// the device with the header's own layout constants: it polls the guards, decodes the line, writes the flags, then `done`.
// Built with -fsanitize=address,undefined and run as a program of its own by tests/test_mailbox_host.py.
#include "evs_mailbox.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
using namespace evs;
using L = MailboxLayout;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

struct Seen {   // what the fake server decoded from one accepted line
    unsigned want; bool by_addr; std::vector<unsigned> ids;
    unsigned long long ids_addr, stride, out; int slot;
};
struct Device {
    alignas(128) unsigned block[L::kBlockBytes / 4] = {};
    int T = 0, n_slots = 1;
    std::vector<Seen> seen;
    std::atomic<int> polls_rejected{0};   // lines looked at whose guards did not all hold the number awaited
    volatile unsigned *w() { return block; }
    // the server: enter (seq = done, alive = 1), serve until the stop word, leave (alive = 0)
    void run() {
        volatile unsigned *req = w() + L::kReqLine, *ans = w() + L::kAnsLine;
        unsigned seq = ans[L::kDoneWord];
        ans[L::kAliveWord] = 1u;
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
        for (;;) {
            const unsigned want = (seq + 1u) & L::kSeqMask;
            unsigned word[L::kLineWords + 1];
            bool stop = false;
            for (;;) {
                for (int k = 0; k <= L::kLineWords; k++) word[k] = req[k];   // (the line and the stop word behind it)
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                unsigned long long lanes = 0;
                for (int k = 0; k < L::kLineWords; k++) if ((word[k] & L::kSeqMask) == want) lanes |= 1ull << k;
                if ((lanes & L::kGuardLanes) == L::kGuardLanes) break;
                if (lanes & L::kGuardLanes) polls_rejected++;
                if (word[L::kStopWord] != 0u) { stop = true; break; }
                std::this_thread::yield();
            }
            if (stop) break;
            for (int k = 0; k < L::kLineWords; k++) word[k] = req[k];   // all guards held: what lies before them is complete
            Seen s{};
            s.want = want; s.by_addr = (word[L::kGuardWords[0]] & L::kByAddrBit) != 0u;
            for (int g : L::kGuardWords) CHECK(((word[g] & L::kByAddrBit) != 0u) == s.by_addr && (word[g] & L::kSeqMask) == want);
            if (s.by_addr) {
                s.ids_addr = ((unsigned long long)word[L::kIdsAddrHi] << 32) | word[L::kIdsAddrLo];
                s.stride = word[L::kIdsStride];
                s.out = ((unsigned long long)word[L::kOutByAddrHi] << 32) | word[L::kOutByAddrLo];
            } else {
                for (int t = 0; t < T; t++) s.ids.push_back(word[L::id_word(t)]);
                if (T <= L::kMaxTablesTo) s.out = ((unsigned long long)word[L::kOutHi] << 32) | word[L::kOutLo];
            }
            s.slot = (int)(want % (unsigned)n_slots);
            seen.push_back(s);
            volatile unsigned char *fl = reinterpret_cast<volatile unsigned char *>(ans);
            for (int t = 0; t < T; t++) fl[t] = (unsigned char)(s.by_addr ? 200 + t : (s.ids[t] * 7u + want) & 0xffu);
            __atomic_thread_fence(__ATOMIC_RELEASE);
            seq = want;
            ans[L::kDoneWord] = seq;
        }
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
        ans[L::kAliveWord] = 0u;
    }
};

static void id_words_and_destinations() {
    for (int T : {1, 7, 8, 14, 26, 27, 28}) {
        for (int t = 0; t < T; t++) for (int g : L::kGuardWords) CHECK(L::id_word(t) != g && L::id_word(t) < L::kLineWords);
        Device dev; dev.T = T; dev.n_slots = 4;
        MailboxHost mb; mb.line = dev.w(); mb.slots = 4;
        std::thread th([&] { dev.run(); });
        std::vector<int32_t> rows(T);
        std::vector<unsigned char> flags(T);
        int idle_calls = 0;
        auto on_idle = [&](bool) { idle_calls++; return 0; };
        for (int r = 0; r < 40; r++) {
            for (int t = 0; t < T; t++) rows[t] = (int32_t)(0x7f000000u + 1000u * r + t);   // (large ids: no word looks like a sequence number)
            const bool to = T <= L::kMaxTablesTo && (r & 1);
            const bool by_addr = to && (r % 4 == 3);
            const unsigned long long out = to ? 0x00007f1234560000ull + 64ull * r : 0ull, ida = 0x00007e00aabb0000ull + 8ull * r;
            const MailboxHost::Posted p = by_addr ? mb.post(T, nullptr, reinterpret_cast<const void *>(ida), 5 + r, reinterpret_cast<const void *>(out))
                                                  : mb.post(T, rows.data(), nullptr, 0, reinterpret_cast<const void *>(out));
            CHECK(p.want == (unsigned)(r + 1) && p.slot == (r + 1) % 4);
            CHECK(mb.await(p.want, flags.data(), T, on_idle) == 0);
            CHECK((int)dev.seen.size() == r + 1);
            const Seen &s = dev.seen.back();
            CHECK(s.want == p.want && s.slot == p.slot && s.by_addr == by_addr && s.out == out);
            if (by_addr) CHECK(s.ids_addr == ida && s.stride == (unsigned long long)(5 + r));
            else for (int t = 0; t < T; t++) CHECK(s.ids[t] == (unsigned)rows[t]);
            for (int t = 0; t < T; t++) CHECK(flags[t] == (unsigned char)(by_addr ? 200 + t : ((unsigned)rows[t] * 7u + p.want) & 0xffu));
            if (!by_addr && T > L::kMaxTablesTo) {   // words 29 / 30 are ids there
                CHECK(mb.line[L::kOutLo] == (unsigned)rows[L::kMaxTablesTo]);
                if (T == L::kMaxTables) CHECK(mb.line[L::kOutHi] == (unsigned)rows[L::kMaxTablesTo + 1]);
            }
        }
        mb.set_stop(true);
        th.join();
        mb.set_stop(false);
        CHECK(dev.w()[L::kAnsLine + L::kAliveWord] == 0u);   // the stop word made it leave and clear `alive`
        (void)idle_calls;
    }
}

static void three_of_four_guards() {
    Device dev; dev.T = 8;
    MailboxHost mb; mb.line = dev.w(); mb.slots = 1;
    std::thread th([&] { dev.run(); });
    while (dev.w()[L::kAnsLine + L::kAliveWord] == 0u) std::this_thread::yield();
    for (int missing = 0; missing < 4; missing++) {
        const size_t before = dev.seen.size();
        const int rejected0 = dev.polls_rejected.load();
        const unsigned want = mb.next_want();
        for (int t = 0; t < 8; t++) dev.w()[L::id_word(t)] = 0x7e000000u + t;
        __atomic_thread_fence(__ATOMIC_RELEASE);
        for (int g = 0; g < 4; g++) if (g != missing) dev.w()[L::kGuardWords[g]] = want;
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
        while (dev.polls_rejected.load() < rejected0 + 50) std::this_thread::yield();   // the server has looked at it 50 times
        CHECK(dev.seen.size() == before && dev.w()[L::kAnsLine + L::kDoneWord] != want);
        // the whole line, through the protocol: now it is taken
        std::vector<int32_t> rows(8, 5);
        unsigned char flags[8];
        const MailboxHost::Posted p = mb.post(8, rows.data(), nullptr, 0, nullptr);
        CHECK(p.want == want && mb.await(p.want, flags, 8, [](bool) { return 0; }) == 0);
        CHECK(dev.seen.size() == before + 1);
    }
    mb.set_stop(true);
    th.join();
}

static void slot_order_and_wrap() {
    for (int n_slots : {1, 4}) {
        Device dev; dev.T = 7; dev.n_slots = n_slots;
        dev.w()[L::kAnsLine + L::kDoneWord] = L::kSeqMask - 2u;   // host and server both start two requests before the wrap
        MailboxHost mb; mb.line = dev.w(); mb.slots = n_slots; mb.seq = L::kSeqMask - 2u;
        std::thread th([&] { dev.run(); });
        std::vector<int32_t> rows(7, 3);
        unsigned char flags[7];
        const unsigned expect[5] = {0x7ffffffeu, 0x7fffffffu, 0u, 1u, 2u};
        for (int r = 0; r < 5; r++) {
            const int slot_before = mb.next_slot();
            const MailboxHost::Posted p = mb.post(7, rows.data(), nullptr, 0, nullptr);
            CHECK(p.want == expect[r] && p.slot == (int)(expect[r] % (unsigned)n_slots) && p.slot == slot_before);
            CHECK(mb.await(p.want, flags, 7, [](bool) { return 0; }) == 0);
            CHECK(dev.seen.back().want == expect[r] && dev.seen.back().slot == p.slot && mb.seq == expect[r]);
        }
        mb.set_stop(true);
        th.join();
    }
}

static void on_idle_rules() {
    // nobody alive: on_idle runs (first spin, then every 64th), and the server it starts answers
    {
        Device dev; dev.T = 14;
        MailboxHost mb; mb.line = dev.w(); mb.slots = 1;
        std::vector<int32_t> rows(14, 9);
        unsigned char flags[14];
        std::thread th;
        int calls = 0;
        const MailboxHost::Posted p = mb.post(14, rows.data(), nullptr, 0, nullptr);
        CHECK(mb.await(p.want, flags, 14, [&](bool gave_up) { CHECK(!gave_up); if (calls++ == 2) th = std::thread([&] { dev.run(); }); return 0; }) == 0);
        CHECK(calls >= 3 && th.joinable());
        // a server is alive: on_idle is not called, however long the answer takes
        int calls_alive = 0;
        for (int r = 0; r < 200; r++) {
            const MailboxHost::Posted q = mb.post(14, rows.data(), nullptr, 0, nullptr);
            CHECK(mb.await(q.want, flags, 14, [&](bool) { calls_alive++; return 0; }) == 0);
        }
        CHECK(calls_alive == 0);
        mb.set_stop(true);
        th.join();
        mb.set_stop(false);
        // nobody alive again, and on_idle fails: its code comes back and seq is the number last ANSWERED
        const unsigned answered = mb.seq;
        const MailboxHost::Posted f = mb.post(14, rows.data(), nullptr, 0, nullptr);
        CHECK(mb.seq == f.want && f.want == answered + 1u);
        CHECK(mb.await(f.want, flags, 14, [&](bool) { return -7; }) == -7);
        CHECK(mb.seq == answered && mb.next_want() == f.want);
        // the next request reuses the number, and a fresh server (which reads `done` on entry) agrees
        std::thread th2([&] { dev.run(); });
        const MailboxHost::Posted g = mb.post(14, rows.data(), nullptr, 0, nullptr);
        CHECK(g.want == f.want && mb.await(g.want, flags, 14, [](bool) { return 0; }) == 0);
        CHECK(dev.seen.back().want == g.want);
        mb.set_stop(true);
        th2.join();
    }
}

int main() {
    id_words_and_destinations();
    three_of_four_guards();
    slot_order_and_wrap();
    on_idle_rules();
    printf("mailbox host check ok\n");
    return 0;
}
