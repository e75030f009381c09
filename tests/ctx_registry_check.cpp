// Driver for tests/test_ctx_registry.py: the context registry of the C ABI (csrc/ctx_registry.h) on a fake context, built with
// -fsanitize=thread.  Prints one "ok <check>" line per passed check; exits non-zero at the first failed one.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include "ctx_registry.h"

namespace {

struct Fake {
    std::mutex mu;
    bool dead = false;
    long calls = 0;           // written only under mu: a call admitted without the lock is a data race ThreadSanitizer reports
};

std::atomic<int> deleted{0};
std::atomic<int> holders{0};            // threads inside an admitted call
std::atomic<int> deleted_with_holders{0};
void count_delete(Fake* f) {
    if (holders.load() != 0) ++deleted_with_holders;
    ++deleted;
    delete f;
}

void check(bool ok, const char* what) {
    if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what); std::exit(1); }
    std::printf("ok %s\n", what);
    std::fflush(stdout);
}

// several threads admit and release in a loop while another thread retires the context
void concurrent_retire() {
    efe::CtxRegistry<Fake> reg(count_delete);
    Fake* f = new Fake();
    reg.insert(f);
    std::atomic<bool> retired{false}, stop{false};
    std::atomic<int> admitted{0}, after_retire{0};
    std::vector<std::thread> ts;
    for (int t = 0; t < 4; ++t)
        ts.emplace_back([&] {
            while (!stop.load()) {
                const bool was_retired = retired.load();
                auto a = reg.admit(f);
                if (!a) continue;
                ++holders;
                if (was_retired) ++after_retire;
                ++a.ctx->calls;
                ++admitted;
                --holders;
            }
        });
    while (admitted.load() < 2000) std::this_thread::yield();
    std::thread retirer([&] { reg.retire(f); retired = true; });
    retirer.join();
    std::this_thread::sleep_for(std::chrono::milliseconds(50));       // admissions keep being attempted after the retirement
    stop = true;
    for (auto& t : ts) t.join();
    check(admitted.load() >= 2000, "concurrent: admissions succeed while the context is live");
    check(after_retire.load() == 0, "concurrent: no admission succeeds after retirement returns");
    check(!reg.alive(f), "concurrent: a retired context is not alive");
    check(deleted.load() == 1, "concurrent: the deleter ran exactly once");
    check(deleted_with_holders.load() == 0, "concurrent: the deleter ran after the last holder was gone");
    deleted = 0;
}

// retirement waits for the call that holds the context's lock; the deleter runs once, when the last owner lets go
void retire_waits_for_holder() {
    efe::CtxRegistry<Fake> reg(count_delete);
    Fake* f = new Fake();
    reg.insert(f);
    check(reg.alive(f), "holder: an inserted context is alive");
    std::atomic<bool> holding{false}, released{false};
    std::thread holder([&] {
        auto a = reg.admit(f);
        if (!a) return;
        ++holders;
        holding = true;
        std::this_thread::sleep_for(std::chrono::milliseconds(300));
        ++a.ctx->calls;
        released = true;
        --holders;
    });
    while (!holding.load()) std::this_thread::yield();
    reg.retire(f);
    check(released.load(), "holder: retirement did not return while an admitted call held the lock");
    holder.join();
    check(deleted.load() == 1 && deleted_with_holders.load() == 0, "holder: the deleter ran once, after the holder let go");
    check(!reg.admit(f), "holder: a retired handle is refused");
    reg.retire(f);
    check(deleted.load() == 1, "holder: a second retirement is a no-op");
    deleted = 0;
}

// an admission that took ownership before the retirement removed the entry gets the lock only after it: the state it then finds --
// still reachable, marked dead -- is refused
void dead_is_refused() {
    efe::CtxRegistry<Fake> reg(count_delete);
    Fake* f = new Fake();
    reg.insert(f);
    { std::lock_guard<std::mutex> l(f->mu); f->dead = true; }
    check(!reg.admit(f), "dead: a context marked dead is refused");
    reg.retire(f);
    check(deleted.load() == 1, "dead: retiring it runs the deleter once");
    deleted = 0;
}

// handles that were never inserted are refused by value: never dereferenced (0x1000 would fault, a stack object is a live T)
void unknown_handles() {
    efe::CtxRegistry<Fake> reg(count_delete);
    Fake on_stack;
    const Fake* made_up = reinterpret_cast<const Fake*>(static_cast<std::uintptr_t>(0x1000));
    check(!reg.admit(nullptr) && !reg.alive(nullptr), "unknown: nullptr is refused");
    check(!reg.admit(made_up) && !reg.alive(made_up), "unknown: a made-up pointer is refused");
    check(!reg.admit(&on_stack), "unknown: an object that was never inserted is refused");
    reg.retire(made_up);
    reg.retire(nullptr);
    check(deleted.load() == 0, "unknown: retiring an unknown handle deletes nothing");
}

}  // namespace

int main() {
    unknown_handles();
    retire_waits_for_holder();
    dead_is_refused();
    concurrent_retire();
    std::printf("ALL OK\n");
    return 0;
}
