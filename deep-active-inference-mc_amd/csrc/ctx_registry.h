// Registry of the live contexts behind the C ABI's handles: plain C++17, no HIP (tests/ctx_registry_check.cpp runs it under
// ThreadSanitizer).  T has a `std::mutex mu` and a `bool dead`; the registry owns each context through a shared_ptr with the given deleter.
//   admission  : the handle is looked up by value, never dereferenced (the registry mutex is held for the lookup only); a hit takes shared
//                ownership, then T::mu, then checks `dead`.  A miss or a dead context is a refusal.
//   retirement : removes the entry (later admissions miss), then takes T::mu -- waiting for the call that holds it -- and sets `dead` for
//                admissions that got ownership before the removal.  The deleter runs when the last owner lets go.
#pragma once
#include <memory>
#include <mutex>
#include <unordered_map>

namespace efe {

template <class T>
class CtxRegistry {
public:
    explicit CtxRegistry(void (*del)(T*)) : del_(del) {}

    // an admitted call: ownership and T::mu until it goes out of scope (the lock is released first)
    struct Admission {
        std::shared_ptr<T> ctx;
        std::unique_lock<std::mutex> lock;
        explicit operator bool() const { return ctx != nullptr; }
    };
    void insert(T* ctx) { std::lock_guard<std::mutex> l(mu_); live_.emplace(ctx, std::shared_ptr<T>(ctx, del_)); }
    bool alive(const T* ctx) { std::lock_guard<std::mutex> l(mu_); return live_.count(ctx) != 0; }

    Admission admit(const T* ctx) {
        std::shared_ptr<T> sp = find(ctx, false);
        if (!sp) return {};
        std::unique_lock<std::mutex> lock(sp->mu);
        if (sp->dead) return {};                 // retired while this call waited for the lock
        return {std::move(sp), std::move(lock)};
    }
    // a handle that is not live (retired before, never inserted) is ignored
    void retire(const T* ctx) {
        std::shared_ptr<T> sp = find(ctx, true);
        if (!sp) return;
        std::lock_guard<std::mutex> l(sp->mu);
        sp->dead = true;
    }

private:
    std::shared_ptr<T> find(const T* ctx, bool remove) {
        std::lock_guard<std::mutex> l(mu_);
        auto it = live_.find(ctx);
        if (it == live_.end()) return nullptr;
        std::shared_ptr<T> sp = it->second;
        if (remove) live_.erase(it);
        return sp;
    }

    void (*del_)(T*);
    std::mutex mu_;
    std::unordered_map<const T*, std::shared_ptr<T>> live_;
};

}  // namespace efe
