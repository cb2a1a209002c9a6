// Stand-alone check of the carried order's structural key (raytracingincuda_amd/csrc/library/order_key.h), built with
// -fsanitize=address,undefined by tests/test_order_key.py and run directly: equal keys match, every single field that differs
// gives a mismatch, and CarriedOrder hands an order out only while it is valid and for the key it was stored with.
#include <cstdio>
#include <cstring>
#include <vector>

#include "order_key.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static OrderKey from_words(const std::vector<int32_t>& w) {
    OrderKey k;
    std::memcpy(&k, w.data(), sizeof k);
    return k;
}

int main() {
    // the headline launch: 1920 x 1080, one rank, 100 spp, 50 bounces, fp32, sorted, grid source, 64 lanes, 1280 workgroups, 32400 pools
    const OrderKey base = {1920, 1080, 0, 1, 8, 100, 50, 32, 2, 3, 64, 1280, 32400, 0, 2, 1, 1};
    std::vector<int32_t> words(ORDER_KEY_FIELDS);
    std::memcpy(words.data(), &base, sizeof base);
    CHECK(order_key_equal(base, base));
    CHECK(order_key_equal(base, from_words(words)));
    CHECK(order_key_equal(OrderKey{}, OrderKey{}));
    CHECK(!order_key_equal(base, OrderKey{}));
    // every field on its own: another value, the smallest change, a sign flip, the extremes
    for (int f = 0; f < ORDER_KEY_FIELDS; ++f) {
        for (const int32_t other : {words[f] + 1, words[f] - 1, -words[f] - 1, (int32_t)0x7fffffff, (int32_t)(-0x7fffffff - 1)}) {
            std::vector<int32_t> w = words;
            w[f] = other;
            const OrderKey k = from_words(w);
            CHECK(!order_key_equal(base, k));
            CHECK(!order_key_equal(k, base));
            CHECK(order_key_equal(k, k));
        }
    }
    // two fields swapped between neighbours (W <-> local_rows, solo_waves <-> solo_lanes) is a different launch
    for (const int f : {0, 13}) {
        std::vector<int32_t> w = words;
        std::swap(w[f], w[f + 1]);
        CHECK(!order_key_equal(base, from_words(w)));
    }

    CarriedOrder c;
    CHECK(!c.usable(base));                       // nothing stored
    CHECK(!c.usable(OrderKey{}));                 // ... not even for the all-zero key a fresh handle holds
    c.store(base);
    CHECK(c.usable(base));
    OrderKey shard = base;
    shard.rank = 1; shard.nranks = 2; shard.local_rows = 540;
    CHECK(!c.usable(shard));
    CHECK(c.usable(base));                        // a refused key leaves the stored one alone
    c.clear();
    CHECK(!c.usable(base));
    c.store(shard);
    CHECK(c.usable(shard) && !c.usable(base));
    const CarriedOrder copy = c;                  // rtiow_set_camera with the identical camera puts a copy back
    c.clear();
    c = copy;
    CHECK(c.usable(shard));

    std::printf("%d order-key failure(s)\n", failures);
    return failures ? 1 : 0;
}
