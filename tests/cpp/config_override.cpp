// The thread-local override of the behaviour switches (csrc/tdr_config.h): host code only, no device is touched.
//   * an installed TdrConfigScope is what tdr_cfg() returns on its thread;
//   * a second thread reads the process-wide values throughout;
//   * a configuring call made while a scope is installed lands in the process-wide struct and survives the scope;
//   * nested scopes unwind in order.
// Prints "ok"; a failed check prints its line and exits 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "tdr.h"
#include "tdr_config.h"

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("config_override.cpp:%d: %s\n", __LINE__, #cond);  \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

int main() {
  const TdrConfig before = tdr_cfg();
  CHECK(before.su_mode == 1 && before.su_span == 16.f && !before.su_span_fixed && before.cart_seg_rows == 32);
  CHECK(tdr_config_shift_uniform(-1) == 1 && tdr_config_tuning("cart_seg_rows", -1) == 32);

  // the other thread: polls while the main thread goes through its scopes, and must see the process-wide values only
  // stage 0: scopes being installed and removed; 3: parked (the main thread configures: one thread at a time, tdr_config.h);
  // 1: the main thread has set a switch; 2: stop
  std::atomic<int> stage{0};
  std::atomic<long> polls0{0}, polls1{0};
  std::atomic<bool> moved{false}, parked{false};
  std::thread other([&] {
    for (;;) {
      const int s = stage.load();
      if (s == 2) break;
      if (s == 3) { parked = true; continue; }
      const TdrConfig& c = tdr_cfg();
      if (c.su_mode != 1 || c.su_span != 16.f || c.su_span_fixed || c.ray_split != 0 || c.cart_seg_rows != (s == 0 ? 32 : 8))
        moved = true;
      (s == 0 ? polls0 : polls1)++;
    }
  });
  while (polls0.load() == 0) std::this_thread::yield();

  {
    TdrConfig a = tdr_cfg();
    a.su_mode = 2; a.su_span = 1e-6f; a.su_span_fixed = true; a.cart_seg_rows = 0;
    TdrConfigScope sa(a);
    CHECK(tdr_cfg().su_mode == 2 && tdr_cfg().su_span == 1e-6f && tdr_cfg().su_span_fixed && tdr_cfg().cart_seg_rows == 0);
    // the configuring calls see and change the process-wide struct, never the override
    CHECK(tdr_config_shift_uniform(-1) == 1 && tdr_config_shift_uniform_span(-1.f) == 16.f);
    {
      TdrConfig b = tdr_cfg();   // a copy of the override in force
      CHECK(b.su_mode == 2);
      b.su_mode = 0; b.ray_split = 4;
      TdrConfigScope sb(b);
      CHECK(tdr_cfg().su_mode == 0 && tdr_cfg().ray_split == 4 && tdr_cfg().cart_seg_rows == 0);
      const long seen = polls0.load();
      while (polls0.load() < seen + 100) std::this_thread::yield();   // the other thread reads under two nested scopes
    }
    CHECK(tdr_cfg().su_mode == 2 && tdr_cfg().ray_split == 0 && tdr_cfg().cart_seg_rows == 0);   // back to the outer scope
    stage = 3;
    while (!parked.load()) std::this_thread::yield();
    CHECK(tdr_config_tuning("cart_seg_rows", 9) == 8);    // set under an override: the process-wide value moves ...
    stage = 1;
    CHECK(tdr_cfg().cart_seg_rows == 0);                  // ... this thread still reads its override ...
    const long seen = polls1.load();
    while (polls1.load() < seen + 100) std::this_thread::yield();   // ... and the other thread the new value
  }
  CHECK(tdr_cfg().cart_seg_rows == 8 && tdr_config_tuning("cart_seg_rows", -1) == 8);   // it survives the scope
  CHECK(tdr_cfg().su_mode == 1 && tdr_cfg().su_span == 16.f && !tdr_cfg().su_span_fixed);
  stage = 2;
  other.join();
  CHECK(!moved.load());
  CHECK(polls0.load() > 0 && polls1.load() > 0);
  CHECK(tdr_config_tuning("cart_seg_rows", 32) == 32);
  std::printf("ok\n");
  return 0;
}
