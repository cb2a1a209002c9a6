// order_key.h -- the structural key of a carried hand-out order (launch_render, RTIOW_SCHED_SORTED).
// After a sorted two-phase render h->order (slot -> pixel) and h->slot_of (pixel -> slot) stay valid, and the next render of the same frame
// launches once, in that order, from sample 0.  The order indexes pixels, slots and waves of ONE launch geometry: read on another frame it
// would index out of bounds.  OrderKey names everything that layout depends on; launch_render stores it with the order and compares it on
// every call, whatever the setters did in between.  A mismatch renders in two phases again.
// Plain C++ (no HIP): also built on its own by tests/native/order_key_main.cpp.
#pragma once
#include <cstdint>

struct OrderKey {
    int32_t W, local_rows;                 // the local frame: order entries are (local row << 16 | column), slot_of has W x local_rows entries
    int32_t rank, nranks, strip_rows;      // the shard those rows belong to
    int32_t S, B;                          // samples and bounce limit: prepass length, solo-wave rule
    int32_t precision, schedule, scene_source;
    int32_t lane_cap, blocks, total_pools; // launch geometry: first pools per resident wave, slots of the order
    int32_t solo_waves, solo_lanes;        // the first solo_waves x solo_lanes slots are the solo waves'
    int32_t bounded_f32, staged_stores;    // the kernel pair the launch was sized for; pixels stored by slot (h->staged, h->slot_of)
};
constexpr int ORDER_KEY_FIELDS = 17;
static_assert(sizeof(OrderKey) == ORDER_KEY_FIELDS * sizeof(int32_t), "OrderKey: every field is an int32_t and is compared below");

inline bool order_key_equal(const OrderKey& a, const OrderKey& b) {
    return a.W == b.W && a.local_rows == b.local_rows && a.rank == b.rank && a.nranks == b.nranks && a.strip_rows == b.strip_rows &&
           a.S == b.S && a.B == b.B && a.precision == b.precision && a.schedule == b.schedule && a.scene_source == b.scene_source &&
           a.lane_cap == b.lane_cap && a.blocks == b.blocks && a.total_pools == b.total_pools &&
           a.solo_waves == b.solo_waves && a.solo_lanes == b.solo_lanes && a.bounded_f32 == b.bounded_f32 && a.staged_stores == b.staged_stores;
}

// The carried order and its key, as the handle holds them.  store(): a two-phase render has just written the order for `key`.
// usable(): the next launch may read it -- it is there, nothing has overwritten it, and it was laid out for exactly this launch.
struct CarriedOrder {
    bool valid = false;
    OrderKey key{};
    void store(const OrderKey& k) { key = k; valid = true; }
    void clear() { valid = false; }
    bool usable(const OrderKey& k) const { return valid && order_key_equal(key, k); }
};
