// ge_addon.cc — thin N-API binding of include/ge_step.h for the TypeScript/Node host.
//
// Where it sits in the reference: src/app/api/copilotkit/route.ts:22-47 builds a
// LangGraphAgent per request that forwards the room's AgentState over HTTP to the Python
// LangGraph server (agent/langgraph.json:5-8 -> game_agent_v2.py:graph).  A host that wants the
// GPU stepper instead calls this addon (see index.js / index.d.ts and INTEGRATION.md).
// No game logic here: every export is a 1:1 wrapper of a C-ABI entry point; stepping runs on the
// libuv pool (napi_create_async_work) so the event loop is never blocked.
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include <string>
#include <vector>

#include "../../include/ge_step.h"

namespace {

#define NAPI_OK(call)                                                        \
    do {                                                                     \
        if ((call) != napi_ok) {                                             \
            napi_throw_error(env, "GE_NAPI", "N-API call failed: " #call);   \
            return nullptr;                                                  \
        }                                                                    \
    } while (0)

napi_value throw_status(napi_env env, int st, const char *what, const char *detail = nullptr) {
    bool pending = false;
    if (napi_is_exception_pending(env, &pending) == napi_ok && pending) return nullptr;   // e.g. GE_BUSY from batch_arg
    std::string msg = std::string(what) + ": " + ge_strerror(st);
    if (detail && *detail) msg += std::string(" (") + detail + ")";
    char code[16];
    snprintf(code, sizeof code, "GE%d", st);
    napi_throw_error(env, code, msg.c_str());
    return nullptr;
}

bool get_u64(napi_env env, napi_value v, uint64_t *out) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return false;
    if (t == napi_bigint) {
        bool lossless;
        return napi_get_value_bigint_uint64(env, v, out, &lossless) == napi_ok;
    }
    if (t == napi_number) {
        double d;
        if (napi_get_value_double(env, v, &d) != napi_ok || d < 0) return false;
        *out = (uint64_t)d;
        return true;
    }
    return false;
}

bool get_prop_u64(napi_env env, napi_value obj, const char *name, uint64_t *out, uint64_t dflt) {
    bool has = false;
    napi_value v;
    *out = dflt;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return true;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return false;
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (t == napi_undefined || t == napi_null) return true;
    if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); *out = b; return true; }
    return get_u64(env, v, out);
}

// What a batch External holds.  The C handle is not thread-safe (ge_step.h), so while an async step owns
// it on a libuv worker (`busy`) every other entry point refuses it instead of racing, and the worker keeps
// a reference on the External so that the garbage collector cannot finalize it mid-step.
struct BatchBox {
    ge_batch *b = nullptr;
    bool busy = false;
};
void finalize_batch(napi_env, void *data, void *) {
    BatchBox *box = static_cast<BatchBox *>(data);
    if (box->b) ge_batch_destroy(box->b);
    delete box;
}
void finalize_table(napi_env, void *data, void *) { free(data); }

// compileTable(dslJson: string, rounds?: number): External<ge_game_table>
napi_value CompileTable(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 1) return throw_status(env, GE_ERR_ARG, "compileTable");
    size_t len = 0;
    NAPI_OK(napi_get_value_string_utf8(env, argv[0], nullptr, 0, &len));
    std::string json(len, '\0');
    NAPI_OK(napi_get_value_string_utf8(env, argv[0], &json[0], len + 1, &len));
    uint64_t rounds = 1;
    if (argc > 1 && !get_u64(env, argv[1], &rounds)) rounds = 1;
    ge_game_table *t = static_cast<ge_game_table *>(calloc(1, sizeof(ge_game_table)));
    char err[512];
    int st = ge_table_compile_json(json.data(), json.size(), (int)rounds, t, err, sizeof err);
    if (st != GE_OK) { free(t); return throw_status(env, st, "compileTable", err); }
    napi_value ext;
    NAPI_OK(napi_create_external(env, t, finalize_table, nullptr, &ext));
    return ext;
}

// tableInfo(table): { pack, rounds, minPlayers, roleNames[], fieldNames[], phases:[{id,name,completion,act,effect,nBranches}], initFields[] }
napi_value TableInfo(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_game_table *t = nullptr;
    if (argc < 1 || napi_get_value_external(env, argv[0], reinterpret_cast<void **>(&t)) != napi_ok || !t)
        return throw_status(env, GE_ERR_ARG, "tableInfo");
    napi_value out, phases, roles, v;
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_create_int32(env, t->pack, &v)); NAPI_OK(napi_set_named_property(env, out, "pack", v));
    NAPI_OK(napi_create_int32(env, t->rounds, &v)); NAPI_OK(napi_set_named_property(env, out, "rounds", v));
    NAPI_OK(napi_create_int32(env, t->min_players, &v)); NAPI_OK(napi_set_named_property(env, out, "minPlayers", v));
    NAPI_OK(napi_create_array_with_length(env, 5, &roles));
    for (uint32_t i = 0; i < 5; i++) {
        NAPI_OK(napi_create_string_utf8(env, t->role_names[i], NAPI_AUTO_LENGTH, &v));
        NAPI_OK(napi_set_element(env, roles, i, v));
    }
    NAPI_OK(napi_set_named_property(env, out, "roleNames", roles));
    napi_value fields;                     // slot (GE_WW_* / GE_TT_*) -> the DSL's own field name, "" = not declared
    NAPI_OK(napi_create_array_with_length(env, GE_MAX_SLOTS, &fields));
    for (uint32_t i = 0; i < GE_MAX_SLOTS; i++) {
        NAPI_OK(napi_create_string_utf8(env, t->field_names[i], NAPI_AUTO_LENGTH, &v));
        NAPI_OK(napi_set_element(env, fields, i, v));
    }
    NAPI_OK(napi_set_named_property(env, out, "fieldNames", fields));
    NAPI_OK(napi_create_array_with_length(env, t->n_phases, &phases));
    for (int i = 0; i < t->n_phases; i++) {
        napi_value ph;
        NAPI_OK(napi_create_object(env, &ph));
        NAPI_OK(napi_create_int32(env, t->rows[i].phase_id, &v)); NAPI_OK(napi_set_named_property(env, ph, "id", v));
        NAPI_OK(napi_create_string_utf8(env, t->rows[i].name, NAPI_AUTO_LENGTH, &v)); NAPI_OK(napi_set_named_property(env, ph, "name", v));
        NAPI_OK(napi_create_int32(env, t->rows[i].completion, &v)); NAPI_OK(napi_set_named_property(env, ph, "completion", v));
        NAPI_OK(napi_create_int32(env, t->rows[i].act, &v)); NAPI_OK(napi_set_named_property(env, ph, "act", v));
        NAPI_OK(napi_create_int32(env, t->rows[i].effect, &v)); NAPI_OK(napi_set_named_property(env, ph, "effect", v));
        NAPI_OK(napi_create_int32(env, t->rows[i].n_branches, &v)); NAPI_OK(napi_set_named_property(env, ph, "nBranches", v));
        NAPI_OK(napi_set_element(env, phases, i, ph));
    }
    NAPI_OK(napi_set_named_property(env, out, "phases", phases));
    napi_value init;                       // player_states_template in canonical field order (what a fresh room's players hold)
    NAPI_OK(napi_create_array_with_length(env, 12, &init));
    for (uint32_t i = 0; i < 12; i++) {
        NAPI_OK(napi_create_uint32(env, t->init_fields[i], &v));
        NAPI_OK(napi_set_element(env, init, i, v));
    }
    NAPI_OK(napi_set_named_property(env, out, "initFields", init));
    return out;
}

// {seed, firstRoom, device, maxFuse, restart, trace, segments:[{table, nPlayers, nRooms, humanMask}]} -> ge_batch_desc; throws and returns false on a bad argument
bool parse_desc(napi_env env, napi_value obj, const char *what, ge_batch_desc *out) {
    ge_batch_desc &d = *out;
    memset(&d, 0, sizeof d);
    uint64_t dev = 0, fuse = 0, restart = 0, trace = 0;
    if (!get_prop_u64(env, obj, "seed", &d.seed, 0) || !get_prop_u64(env, obj, "firstRoom", &d.first_room, 0) ||
        !get_prop_u64(env, obj, "device", &dev, 0) || !get_prop_u64(env, obj, "maxFuse", &fuse, 0) ||
        !get_prop_u64(env, obj, "restart", &restart, 0) || !get_prop_u64(env, obj, "trace", &trace, 0)) {
        throw_status(env, GE_ERR_ARG, what);
        return false;
    }
    d.device = (int32_t)dev; d.max_fuse = (uint32_t)fuse;
    d.flags = (restart ? GE_FLAG_RESTART : GE_FLAG_NONE) | (trace ? GE_FLAG_TRACE : GE_FLAG_NONE);
    napi_value segs;
    uint32_t n = 0;
    bool is_arr = false;
    if (napi_get_named_property(env, obj, "segments", &segs) != napi_ok ||
        napi_is_array(env, segs, &is_arr) != napi_ok || !is_arr ||
        napi_get_array_length(env, segs, &n) != napi_ok || n == 0 || n > GE_MAX_SEGMENTS) {
        throw_status(env, GE_ERR_ARG, what, "segments");
        return false;
    }
    d.n_segments = n;
    for (uint32_t k = 0; k < n; k++) {
        napi_value sg, tv;
        uint64_t np = 0, nr = 0, hm = 0;
        ge_game_table *t = nullptr;
        if (napi_get_element(env, segs, k, &sg) != napi_ok ||
            napi_get_named_property(env, sg, "table", &tv) != napi_ok ||
            napi_get_value_external(env, tv, reinterpret_cast<void **>(&t)) != napi_ok || !t ||
            !get_prop_u64(env, sg, "nPlayers", &np, 0) || !get_prop_u64(env, sg, "nRooms", &nr, 0) ||
            !get_prop_u64(env, sg, "humanMask", &hm, 0)) {
            throw_status(env, GE_ERR_ARG, what, "segment");
            return false;
        }
        d.seg[k].table = t; d.seg[k].n_players = (uint32_t)np; d.seg[k].n_rooms = nr; d.seg[k].human_mask = (uint32_t)hm;
    }
    return true;
}

// createBatch({seed, firstRoom, device, maxFuse, restart, segments:[{table, nPlayers, nRooms}]}): External<ge_batch>
napi_value CreateBatch(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 1) return throw_status(env, GE_ERR_ARG, "createBatch");
    ge_batch_desc d;
    if (!parse_desc(env, argv[0], "createBatch", &d)) return nullptr;
    ge_batch *b = nullptr;
    int st = ge_batch_create(&d, &b);
    if (st != GE_OK) return throw_status(env, st, "createBatch");
    BatchBox *box = new BatchBox();
    box->b = b;
    napi_value ext;
    if (napi_create_external(env, box, finalize_batch, nullptr, &ext) != napi_ok) {
        ge_batch_destroy(b);
        delete box;
        napi_throw_error(env, "GE_NAPI", "napi_create_external failed");
        return nullptr;
    }
    return ext;
}

BatchBox *box_arg(napi_env env, napi_value v) {
    BatchBox *box = nullptr;
    if (napi_get_value_external(env, v, reinterpret_cast<void **>(&box)) != napi_ok) return nullptr;
    return box;
}

// the handle of a batch that is alive and not owned by an async step; throws and returns null otherwise
ge_batch *batch_arg(napi_env env, napi_value v) {
    BatchBox *box = box_arg(env, v);
    if (!box || !box->b) return nullptr;
    if (box->busy) {
        napi_throw_error(env, "GE_BUSY", "an async step() of this batch is in flight: await it first (a ge_batch handle is not thread-safe)");
        return nullptr;
    }
    return box->b;
}

struct StepWork {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref keep;            // the External: alive until the worker is done
    BatchBox *box;
    uint32_t turns;
    int status;
};

void step_execute(napi_env, void *data) {
    StepWork *w = static_cast<StepWork *>(data);
    w->status = ge_batch_step(w->box->b, w->turns, nullptr);
    if (w->status == GE_OK) w->status = ge_batch_sync(w->box->b);
}

void step_complete(napi_env env, napi_status, void *data) {
    StepWork *w = static_cast<StepWork *>(data);
    w->box->busy = false;
    ge_batch *const batch_of_w = w->box->b;
    napi_value v;
    if (w->status == GE_OK) {
        uint64_t turn = 0;
        ge_batch_turn(batch_of_w, &turn);
        napi_create_double(env, (double)turn, &v);
        napi_resolve_deferred(env, w->deferred, v);
    } else {
        napi_value msg;
        napi_create_string_utf8(env, ge_strerror(w->status), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &v);
        napi_reject_deferred(env, w->deferred, v);
    }
    napi_delete_async_work(env, w->work);
    napi_delete_reference(env, w->keep);          // last: from here on the External may be collected
    delete w;
}

// step(batch, nTurns): Promise<number /* turn counter */>
napi_value Step(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t turns = 1;
    if (!b || (argc > 1 && !get_u64(env, argv[1], &turns))) return throw_status(env, GE_ERR_ARG, "step");
    StepWork *w = new StepWork();
    w->box = box_arg(env, argv[0]); w->turns = (uint32_t)turns; w->status = GE_OK;
    napi_value promise, name;
    if (napi_create_reference(env, argv[0], 1, &w->keep) != napi_ok) { delete w; return throw_status(env, GE_ERR_ARG, "step"); }
    if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
        napi_create_string_utf8(env, "ge_batch_step", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_async_work(env, nullptr, name, step_execute, step_complete, w, &w->work) != napi_ok) {
        napi_delete_reference(env, w->keep);
        delete w;
        return throw_status(env, GE_ERR_ARG, "step");
    }
    w->box->busy = true;
    if (napi_queue_async_work(env, w->work) != napi_ok) {
        w->box->busy = false;
        napi_delete_async_work(env, w->work);
        napi_delete_reference(env, w->keep);
        delete w;
        return throw_status(env, GE_ERR_ARG, "step");
    }
    return promise;
}

// stepSync(batch, nTurns): number
napi_value StepSync(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t turns = 1;
    if (!b || (argc > 1 && !get_u64(env, argv[1], &turns))) return throw_status(env, GE_ERR_ARG, "stepSync");
    int st = ge_batch_step(b, (uint32_t)turns, nullptr);
    if (st == GE_OK) st = ge_batch_sync(b);
    if (st != GE_OK) return throw_status(env, st, "stepSync");
    uint64_t turn = 0;
    ge_batch_turn(b, &turn);
    napi_value v;
    NAPI_OK(napi_create_double(env, (double)turn, &v));
    return v;
}

// readRooms(batch, first, count): ArrayBuffer (count * sizeof(ge_room_view) bytes)
napi_value ReadRooms(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t first = 0, count = 0;
    if (!b || argc < 3 || !get_u64(env, argv[1], &first) || !get_u64(env, argv[2], &count))
        return throw_status(env, GE_ERR_ARG, "readRooms");
    void *data = nullptr;
    napi_value buf;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)count * sizeof(ge_room_view), &data, &buf));
    int st = ge_batch_read_rooms(b, first, count, static_cast<ge_room_view *>(data), (size_t)count * sizeof(ge_room_view));
    if (st != GE_OK) return throw_status(env, st, "readRooms");
    return buf;
}

// injectAction(batch, room, playerId, choice): throws GE-1 if the action is not allowed
napi_value InjectAction(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t room = 0, player = 0, choice = 0;
    if (!b || argc < 4 || !get_u64(env, argv[1], &room) || !get_u64(env, argv[2], &player) || !get_u64(env, argv[3], &choice))
        return throw_status(env, GE_ERR_ARG, "injectAction");
    int st = ge_batch_inject_action(b, room, (uint32_t)player, (uint32_t)choice);
    if (st != GE_OK) return throw_status(env, st, "injectAction");
    return nullptr;
}

// injectActions(batch, rooms: BigUint64Array, playerIds: Uint32Array, choices: Uint32Array): Int32Array of per-action status
napi_value InjectActions(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 4) return throw_status(env, GE_ERR_ARG, "injectActions");
    napi_typedarray_type tt[3];
    size_t len[3];
    void *data[3];
    for (int k = 0; k < 3; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "injectActions", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_uint32_array || tt[2] != napi_uint32_array || len[0] != len[1] || len[1] != len[2])
        return throw_status(env, GE_ERR_ARG, "injectActions", "BigUint64Array, Uint32Array, Uint32Array of equal length");
    void *st_data = nullptr;
    napi_value st_buf, st_arr;
    NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(int32_t), &st_data, &st_buf));
    memset(st_data, 0, len[0] * sizeof(int32_t));
    const int st = ge_batch_inject_actions(b, len[0], static_cast<const uint64_t *>(data[0]), static_cast<const uint32_t *>(data[1]),
                                           static_cast<const uint32_t *>(data[2]), static_cast<int32_t *>(st_data));
    if (st != GE_OK) {
        // the return value is the first refused action's status - or a failure of the call itself (allocation, HIP error,
        // too many actions), which leaves the status array untouched: that one must not read as "all applied"
        bool any = false;
        for (size_t k = 0; k < len[0] && !any; k++) any = static_cast<const int32_t *>(st_data)[k] != 0;
        if (!any) return throw_status(env, st, "injectActions");
    }
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, len[0], st_buf, 0, &st_arr));
    return st_arr;
}

// setTurn(batch, turn): restores a checkpoint's turn counter (the RNG is keyed by it)
napi_value SetTurn(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t turn = 0;
    if (!b || argc < 2 || !get_u64(env, argv[1], &turn)) return throw_status(env, GE_ERR_ARG, "setTurn");
    int st = ge_batch_set_turn(b, turn);
    if (st != GE_OK) return throw_status(env, st, "setTurn");
    return nullptr;
}

// writeRooms(batch, first, buffer: ArrayBuffer of ge_room_view): checkpoint restore
napi_value WriteRooms(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t first = 0;
    void *data = nullptr;
    size_t bytes = 0;
    if (!b || argc < 3 || !get_u64(env, argv[1], &first) || napi_get_arraybuffer_info(env, argv[2], &data, &bytes) != napi_ok ||
        bytes % sizeof(ge_room_view) != 0)
        return throw_status(env, GE_ERR_ARG, "writeRooms");
    int st = ge_batch_write_rooms(b, first, bytes / sizeof(ge_room_view), static_cast<const ge_room_view *>(data));
    if (st != GE_OK) return throw_status(env, st, "writeRooms");
    return nullptr;
}

// destroyBatch(batch): releases the device memory now instead of at garbage collection
napi_value DestroyBatch(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    BatchBox *box = argc >= 1 ? box_arg(env, argv[0]) : nullptr;
    if (!box) return throw_status(env, GE_ERR_ARG, "destroyBatch");
    if (box->busy) { napi_throw_error(env, "GE_BUSY", "destroyBatch while an async step() is in flight"); return nullptr; }
    if (box->b) ge_batch_destroy(box->b);
    box->b = nullptr;
    return nullptr;
}

// readEvents(batch, first, count): { nTurns, buffer: ArrayBuffer of count*nTurns ge_turn_event }
napi_value ReadEvents(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    uint64_t first = 0, count = 0;
    if (!b || argc < 3 || !get_u64(env, argv[1], &first) || !get_u64(env, argv[2], &count))
        return throw_status(env, GE_ERR_ARG, "readEvents");
    uint32_t nt = 0;
    int st = ge_batch_read_events(b, first, 0, &nt, nullptr, 0);
    if (st != GE_OK) return throw_status(env, st, "readEvents");
    void *data = nullptr;
    napi_value buf, out, v;
    const size_t bytes = (size_t)count * nt * sizeof(ge_turn_event);
    NAPI_OK(napi_create_arraybuffer(env, bytes, &data, &buf));
    st = ge_batch_read_events(b, first, count, &nt, static_cast<ge_turn_event *>(data), bytes);
    if (st != GE_OK) return throw_status(env, st, "readEvents");
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_create_uint32(env, nt, &v));
    NAPI_OK(napi_set_named_property(env, out, "nTurns", v));
    NAPI_OK(napi_set_named_property(env, out, "buffer", buf));
    return out;
}

// stepRooms(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array): { nTurns: 1, buffer: ArrayBuffer of
// rooms.length ge_turn_event } (readEvents' shape) - one turn of each listed room under its own key and turn
napi_value StepRooms(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 4) return throw_status(env, GE_ERR_ARG, "stepRooms");
    napi_typedarray_type tt[3];
    size_t len[3];
    void *data[3];
    for (int k = 0; k < 3; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "stepRooms", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_biguint64_array || tt[2] != napi_uint32_array || len[0] != len[1] || len[1] != len[2])
        return throw_status(env, GE_ERR_ARG, "stepRooms", "BigUint64Array, BigUint64Array, Uint32Array of equal length");
    void *ev = nullptr;
    napi_value buf, out, v;
    NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(ge_turn_event), &ev, &buf));
    const int st = ge_batch_step_rooms(b, len[0], static_cast<const uint64_t *>(data[0]), static_cast<const uint64_t *>(data[1]),
                                       static_cast<const uint32_t *>(data[2]), static_cast<ge_turn_event *>(ev));
    if (st != GE_OK) return throw_status(env, st, "stepRooms");
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_create_uint32(env, 1, &v));
    NAPI_OK(napi_set_named_property(env, out, "nTurns", v));
    NAPI_OK(napi_set_named_property(env, out, "buffer", buf));
    return out;
}

// stepRoomsPlayout(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array, masks: Uint32Array,
// playoutKeys: BigUint64Array, nRollouts, maxTurns, seed: BigInt, flags): { buffer: ArrayBuffer of rooms.length ge_turn_event,
// decided: Uint32Array } - stepRooms with playout seats (ge_batch_step_rooms_playout, POLICY.md §3d)
napi_value StepRoomsPlayout(napi_env env, napi_callback_info info) {
    size_t argc = 10;
    napi_value argv[10];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 10) return throw_status(env, GE_ERR_ARG, "stepRoomsPlayout");
    napi_typedarray_type tt[5];
    size_t len[5];
    void *data[5];
    for (int k = 0; k < 5; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "stepRoomsPlayout", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_biguint64_array || tt[2] != napi_uint32_array || tt[3] != napi_uint32_array ||
        tt[4] != napi_biguint64_array || len[0] != len[1] || len[1] != len[2] || len[2] != len[3] || len[3] != len[4])
        return throw_status(env, GE_ERR_ARG, "stepRoomsPlayout", "BigUint64Array x 2, Uint32Array x 2, BigUint64Array of equal length");
    uint32_t n_rollouts = 0, max_turns = 0, flags = 0;
    uint64_t seed = 0;
    bool lossless = true;
    if (napi_get_value_uint32(env, argv[6], &n_rollouts) != napi_ok || napi_get_value_uint32(env, argv[7], &max_turns) != napi_ok ||
        napi_get_value_bigint_uint64(env, argv[8], &seed, &lossless) != napi_ok || napi_get_value_uint32(env, argv[9], &flags) != napi_ok)
        return throw_status(env, GE_ERR_ARG, "stepRoomsPlayout", "nRollouts, maxTurns (numbers), seed (BigInt), flags expected");
    void *ev = nullptr, *dec = nullptr;
    napi_value buf, dbuf, darr, out;
    NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(ge_turn_event), &ev, &buf));
    NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(uint32_t), &dec, &dbuf));
    const int st = ge_batch_step_rooms_playout(b, len[0], static_cast<const uint64_t *>(data[0]), static_cast<const uint64_t *>(data[1]),
                                               static_cast<const uint32_t *>(data[2]), static_cast<const uint32_t *>(data[3]),
                                               static_cast<const uint64_t *>(data[4]), n_rollouts, max_turns, seed, flags,
                                               static_cast<ge_turn_event *>(ev), static_cast<uint32_t *>(dec));
    if (st != GE_OK) return throw_status(env, st, "stepRoomsPlayout");
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, len[0], dbuf, 0, &darr));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "buffer", buf));
    NAPI_OK(napi_set_named_property(env, out, "decided", darr));
    return out;
}

// runRooms(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array, maxTurns, until: GE_RUN_UNTIL_* bits, views: boolean):
// { played: Uint32Array, stopped: Uint32Array, events: ArrayBuffer of rooms.length x maxTurns ge_turn_event, views: ArrayBuffer of
// rooms.length x maxTurns ge_room_view | null } - listed rooms played on until a person is needed (ge_batch_run_rooms, POLICY.md
// §3f); entry k's turn t is at k * maxTurns + t, filled below played[k] (zero above).  Synchronous, as stepRoomsPlayout is.
napi_value RunRooms(napi_env env, napi_callback_info info) {
    size_t argc = 7;
    napi_value argv[7];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 7) return throw_status(env, GE_ERR_ARG, "runRooms");
    napi_typedarray_type tt[3];
    size_t len[3];
    void *data[3];
    for (int k = 0; k < 3; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "runRooms", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_biguint64_array || tt[2] != napi_uint32_array || len[0] != len[1] || len[1] != len[2])
        return throw_status(env, GE_ERR_ARG, "runRooms", "BigUint64Array, BigUint64Array, Uint32Array of equal length");
    uint32_t max_turns = 0, until = 0;
    bool want_views = true;
    if (napi_get_value_uint32(env, argv[4], &max_turns) != napi_ok || napi_get_value_uint32(env, argv[5], &until) != napi_ok ||
        napi_get_value_bool(env, argv[6], &want_views) != napi_ok)
        return throw_status(env, GE_ERR_ARG, "runRooms", "maxTurns, until (numbers), views (boolean) expected");
    const size_t n = len[0];
    // the library refuses a call past its caps (after its entry checks): no buffers for it (ArrayBuffers are created zero-filled)
    const size_t slots = (max_turns <= 4096u && (uint64_t)n * max_turns <= (1ull << 20)) ? n * max_turns : 0;
    void *pl = nullptr, *sp = nullptr, *ev = nullptr, *vw = nullptr;
    napi_value pbuf, sbuf, ebuf, vbuf, parr, sarr, out;
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(uint32_t), &pl, &pbuf));
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(uint32_t), &sp, &sbuf));
    NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(ge_turn_event), &ev, &ebuf));
    if (want_views) NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(ge_room_view), &vw, &vbuf));
    else NAPI_OK(napi_get_null(env, &vbuf));
    const int st = ge_batch_run_rooms(b, n, static_cast<const uint64_t *>(data[0]), static_cast<const uint64_t *>(data[1]),
                                      static_cast<const uint32_t *>(data[2]), max_turns, until, static_cast<uint32_t *>(pl),
                                      static_cast<uint32_t *>(sp), static_cast<ge_turn_event *>(ev),
                                      want_views && slots ? static_cast<ge_room_view *>(vw) : nullptr, want_views ? slots * sizeof(ge_room_view) : 0);
    if (st != GE_OK) return throw_status(env, st, "runRooms");
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, pbuf, 0, &parr));
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, sbuf, 0, &sarr));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "played", parr));
    NAPI_OK(napi_set_named_property(env, out, "stopped", sarr));
    NAPI_OK(napi_set_named_property(env, out, "events", ebuf));
    NAPI_OK(napi_set_named_property(env, out, "views", vbuf));
    return out;
}

// findRooms(batch, first, count, want: GE_FIND_* bits, masks: Uint32Array (one word per segment) | null, cap): { hits: ArrayBuffer of
// nHits ge_room_hit (16 B each), nHits, matched } - the rooms of a range that need attention (ge_batch_find_rooms, POLICY.md §3k).
// Synchronous; GE_BUSY from batch_arg.
napi_value FindRooms(napi_env env, napi_callback_info info) {
    size_t argc = 6;
    napi_value argv[6];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 6) return throw_status(env, GE_ERR_ARG, "findRooms");
    int64_t first = 0, count = 0, cap = 0;
    uint32_t want = 0;
    if (napi_get_value_int64(env, argv[1], &first) != napi_ok || napi_get_value_int64(env, argv[2], &count) != napi_ok ||
        napi_get_value_uint32(env, argv[3], &want) != napi_ok || napi_get_value_int64(env, argv[5], &cap) != napi_ok || first < 0 || count < 0 || cap < 0)
        return throw_status(env, GE_ERR_ARG, "findRooms", "first, count, want, cap (non-negative numbers) expected");
    const uint32_t *masks = nullptr;
    napi_valuetype vt;
    NAPI_OK(napi_typeof(env, argv[4], &vt));
    if (vt != napi_null && vt != napi_undefined) {
        napi_typedarray_type tt;
        size_t len, off;
        void *data;
        napi_value ab;
        if (napi_get_typedarray_info(env, argv[4], &tt, &len, &data, &ab, &off) != napi_ok || tt != napi_uint32_array || len < GE_MAX_SEGMENTS)
            return throw_status(env, GE_ERR_ARG, "findRooms", "masks: a Uint32Array of GE_MAX_SEGMENTS words, or null");
        masks = static_cast<const uint32_t *>(data);
    }
    uint64_t n_total = 0;
    (void)ge_batch_n_rooms(b, &n_total);
    // no buffer for a range the library refuses; otherwise min(cap, count) slots, cut to the hits there are
    const uint64_t slots = (uint64_t)first + (uint64_t)count <= n_total ? std::min<uint64_t>((uint64_t)cap, (uint64_t)count) : 0;
    std::vector<ge_room_hit> hits((size_t)slots);
    uint64_t n_hits = 0, n_match = 0;
    const int st = ge_batch_find_rooms(b, (uint64_t)first, (uint64_t)count, want, masks, slots ? hits.data() : nullptr, slots, &n_hits, &n_match);
    if (st != GE_OK) return throw_status(env, st, "findRooms");
    void *dst = nullptr;
    napi_value buf, out, v;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n_hits * sizeof(ge_room_hit), &dst, &buf));
    if (n_hits) memcpy(dst, hits.data(), (size_t)n_hits * sizeof(ge_room_hit));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "hits", buf));
    NAPI_OK(napi_create_double(env, (double)n_hits, &v));
    NAPI_OK(napi_set_named_property(env, out, "nHits", v));
    NAPI_OK(napi_create_double(env, (double)n_match, &v));
    NAPI_OK(napi_set_named_property(env, out, "matched", v));
    return out;
}

// adviseSeats(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array, seats: Uint32Array, nRollouts, maxTurns,
// seed: BigInt, flags: GE_ADVISE_* bits): ArrayBuffer of n ge_advice (224 B each) - the listed seats' legal choices found, played and
// ranked on the device (ge_batch_advise_seats, POLICY.md §3m).  Synchronous; GE_BUSY from batch_arg.
napi_value AdviseSeats(napi_env env, napi_callback_info info) {
    size_t argc = 9;
    napi_value argv[9];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 9) return throw_status(env, GE_ERR_ARG, "adviseSeats");
    napi_typedarray_type tt[4];
    size_t len[4];
    void *data[4];
    for (int k = 0; k < 4; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "adviseSeats", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_biguint64_array || tt[2] != napi_uint32_array || tt[3] != napi_uint32_array ||
        len[1] != len[0] || len[2] != len[0] || len[3] != len[0])
        return throw_status(env, GE_ERR_ARG, "adviseSeats", "BigUint64Array, BigUint64Array, Uint32Array, Uint32Array of equal length");
    uint32_t n_rollouts = 0, max_turns = 0, flags = 0;
    uint64_t seed = 0;
    bool lossless = true;
    if (napi_get_value_uint32(env, argv[5], &n_rollouts) != napi_ok || napi_get_value_uint32(env, argv[6], &max_turns) != napi_ok ||
        napi_get_value_bigint_uint64(env, argv[7], &seed, &lossless) != napi_ok || napi_get_value_uint32(env, argv[8], &flags) != napi_ok)
        return throw_status(env, GE_ERR_ARG, "adviseSeats", "nRollouts, maxTurns (numbers), seed (BigInt), flags expected");
    const size_t n = len[0];
    void *dst = nullptr;
    napi_value buf;
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(ge_advice), &dst, &buf));
    if (n) memset(dst, 0, n * sizeof(ge_advice));
    const int st = ge_batch_advise_seats(b, n, static_cast<const uint64_t *>(data[0]), static_cast<const uint64_t *>(data[1]),
                                         static_cast<const uint32_t *>(data[2]), static_cast<const uint32_t *>(data[3]), n_rollouts, max_turns, seed,
                                         flags, static_cast<ge_advice *>(dst));
    if (st != GE_OK) return throw_status(env, st, "adviseSeats");
    return buf;
}

// setSeats(batch, rooms: BigUint64Array, masks: Uint32Array): undefined - masks[k] becomes the seat mask of room rooms[k]
// (ge_batch_set_seats, POLICY.md §3l).  Synchronous; GE_BUSY from batch_arg.
napi_value SetSeats(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 3) return throw_status(env, GE_ERR_ARG, "setSeats");
    napi_typedarray_type tt[2];
    size_t len[2];
    void *data[2];
    for (int k = 0; k < 2; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "setSeats", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_uint32_array || len[0] != len[1])
        return throw_status(env, GE_ERR_ARG, "setSeats", "BigUint64Array, Uint32Array of equal length");
    const int st = ge_batch_set_seats(b, len[0], static_cast<const uint64_t *>(data[0]), static_cast<const uint32_t *>(data[1]));
    if (st != GE_OK) return throw_status(env, st, "setSeats");
    napi_value undef;
    NAPI_OK(napi_get_undefined(env, &undef));
    return undef;
}

// seats(batch, first, count): Uint32Array - the seat masks of rooms first .. first + count - 1 (ge_batch_get_seats).  Synchronous;
// GE_BUSY from batch_arg.
napi_value Seats(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 3) return throw_status(env, GE_ERR_ARG, "seats");
    int64_t first = 0, count = 0;
    if (napi_get_value_int64(env, argv[1], &first) != napi_ok || napi_get_value_int64(env, argv[2], &count) != napi_ok || first < 0 || count < 0)
        return throw_status(env, GE_ERR_ARG, "seats", "first, count (non-negative numbers) expected");
    uint64_t n_total = 0;
    (void)ge_batch_n_rooms(b, &n_total);
    if ((uint64_t)first + (uint64_t)count > n_total) return throw_status(env, GE_ERR_RANGE, "seats");   // no buffer for a range the library refuses
    void *dst = nullptr;
    napi_value buf, arr;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)count * sizeof(uint32_t), &dst, &buf));
    const int st = ge_batch_get_seats(b, (uint64_t)first, (uint64_t)count, count ? static_cast<uint32_t *>(dst) : nullptr);
    if (st != GE_OK) return throw_status(env, st, "seats");
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, (size_t)count, buf, 0, &arr));
    return arr;
}

// clearSeats(batch): undefined - every room back to its segment's human_mask (ge_batch_clear_seats).  Synchronous; GE_BUSY from batch_arg.
napi_value ClearSeats(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b) return throw_status(env, GE_ERR_ARG, "clearSeats");
    const int st = ge_batch_clear_seats(b);
    if (st != GE_OK) return throw_status(env, st, "clearSeats");
    napi_value undef;
    NAPI_OK(napi_get_undefined(env, &undef));
    return undef;
}

// runRoomsPlayout(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array, masks: Uint32Array, playoutKeys:
// BigUint64Array, nRollouts, playoutMaxTurns, seed: BigInt, flags, maxTurns, until: GE_RUN_UNTIL_* bits, views: boolean): runRooms's
// result plus decided: Uint32Array of rooms.length x maxTurns - runRooms with playout seats (ge_batch_run_rooms_playout, POLICY.md
// §3g); entry k's turn t is at k * maxTurns + t, filled below played[k] (zero above).  Synchronous; GE_BUSY from batch_arg.
napi_value RunRoomsPlayout(napi_env env, napi_callback_info info) {
    size_t argc = 13;
    napi_value argv[13];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 13) return throw_status(env, GE_ERR_ARG, "runRoomsPlayout");
    napi_typedarray_type tt[5];
    size_t len[5];
    void *data[5];
    for (int k = 0; k < 5; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "runRoomsPlayout", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_biguint64_array || tt[2] != napi_uint32_array || tt[3] != napi_uint32_array ||
        tt[4] != napi_biguint64_array || len[0] != len[1] || len[1] != len[2] || len[2] != len[3] || len[3] != len[4])
        return throw_status(env, GE_ERR_ARG, "runRoomsPlayout", "BigUint64Array x 2, Uint32Array x 2, BigUint64Array of equal length");
    uint32_t n_rollouts = 0, pmax = 0, flags = 0, max_turns = 0, until = 0;
    uint64_t seed = 0;
    bool lossless = true, want_views = true;
    if (napi_get_value_uint32(env, argv[6], &n_rollouts) != napi_ok || napi_get_value_uint32(env, argv[7], &pmax) != napi_ok ||
        napi_get_value_bigint_uint64(env, argv[8], &seed, &lossless) != napi_ok || napi_get_value_uint32(env, argv[9], &flags) != napi_ok ||
        napi_get_value_uint32(env, argv[10], &max_turns) != napi_ok || napi_get_value_uint32(env, argv[11], &until) != napi_ok ||
        napi_get_value_bool(env, argv[12], &want_views) != napi_ok)
        return throw_status(env, GE_ERR_ARG, "runRoomsPlayout",
                            "nRollouts, playoutMaxTurns (numbers), seed (BigInt), flags, maxTurns, until (numbers), views (boolean) expected");
    const size_t n = len[0];
    // the library refuses a call past its caps (after its entry checks): no buffers for it (ArrayBuffers are created zero-filled)
    const size_t slots = (max_turns <= 4096u && (uint64_t)n * max_turns <= (1ull << 20)) ? n * max_turns : 0;
    void *pl = nullptr, *sp = nullptr, *dc = nullptr, *ev = nullptr, *vw = nullptr;
    napi_value pbuf, sbuf, dbuf, ebuf, vbuf, parr, sarr, darr, out;
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(uint32_t), &pl, &pbuf));
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(uint32_t), &sp, &sbuf));
    NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(uint32_t), &dc, &dbuf));
    NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(ge_turn_event), &ev, &ebuf));
    if (want_views) NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(ge_room_view), &vw, &vbuf));
    else NAPI_OK(napi_get_null(env, &vbuf));
    const int st = ge_batch_run_rooms_playout(b, n, static_cast<const uint64_t *>(data[0]), static_cast<const uint64_t *>(data[1]),
                                              static_cast<const uint32_t *>(data[2]), static_cast<const uint32_t *>(data[3]),
                                              static_cast<const uint64_t *>(data[4]), n_rollouts, pmax, seed, flags, max_turns, until,
                                              static_cast<uint32_t *>(pl), static_cast<uint32_t *>(sp), static_cast<uint32_t *>(dc),
                                              static_cast<ge_turn_event *>(ev), want_views && slots ? static_cast<ge_room_view *>(vw) : nullptr,
                                              want_views ? slots * sizeof(ge_room_view) : 0);
    if (st != GE_OK) return throw_status(env, st, "runRoomsPlayout");
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, pbuf, 0, &parr));
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, sbuf, 0, &sarr));
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, slots, dbuf, 0, &darr));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "played", parr));
    NAPI_OK(napi_set_named_property(env, out, "stopped", sarr));
    NAPI_OK(napi_set_named_property(env, out, "decided", darr));
    NAPI_OK(napi_set_named_property(env, out, "events", ebuf));
    NAPI_OK(napi_set_named_property(env, out, "views", vbuf));
    return out;
}

// runRoomsForecast(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array, forecastKeys: BigUint64Array, seats:
// Uint32Array, nRollouts, playoutMaxTurns, seed: BigInt, maxTurns, until: GE_RUN_UNTIL_* bits): runRooms's result (with views) plus
// stats: BigUint64Array of rooms.length x (maxTurns + 1) x 77 - runRooms with the forecast of every turn it played
// (ge_batch_run_rooms_forecast, POLICY.md §3i); entry k's point p is at (k * (maxTurns + 1) + p) * 77, filled up to played[k] (zero
// above).  Synchronous; GE_BUSY from batch_arg.
napi_value RunRoomsForecast(napi_env env, napi_callback_info info) {
    size_t argc = 11;
    napi_value argv[11];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 11) return throw_status(env, GE_ERR_ARG, "runRoomsForecast");
    napi_typedarray_type tt[5];
    size_t len[5];
    void *data[5];
    for (int k = 0; k < 5; k++) {
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, "runRoomsForecast", "typed arrays expected");
    }
    if (tt[0] != napi_biguint64_array || tt[1] != napi_biguint64_array || tt[2] != napi_uint32_array || tt[3] != napi_biguint64_array ||
        tt[4] != napi_uint32_array || len[0] != len[1] || len[1] != len[2] || len[2] != len[3] || len[3] != len[4])
        return throw_status(env, GE_ERR_ARG, "runRoomsForecast", "BigUint64Array x 2, Uint32Array, BigUint64Array, Uint32Array of equal length");
    uint32_t n_rollouts = 0, pmax = 0, max_turns = 0, until = 0;
    uint64_t seed = 0;
    bool lossless = true;
    if (napi_get_value_uint32(env, argv[6], &n_rollouts) != napi_ok || napi_get_value_uint32(env, argv[7], &pmax) != napi_ok ||
        napi_get_value_bigint_uint64(env, argv[8], &seed, &lossless) != napi_ok || napi_get_value_uint32(env, argv[9], &max_turns) != napi_ok ||
        napi_get_value_uint32(env, argv[10], &until) != napi_ok)
        return throw_status(env, GE_ERR_ARG, "runRoomsForecast", "nRollouts, playoutMaxTurns (numbers), seed (BigInt), maxTurns, until (numbers) expected");
    const size_t n = len[0];
    // the library refuses a call past its caps (after its entry checks): no buffers for it (ArrayBuffers are created zero-filled)
    const size_t slots = (max_turns <= 4096u && (uint64_t)n * max_turns <= (1ull << 20)) ? n * max_turns : 0;
    const size_t points = (max_turns <= 4096u && (uint64_t)n * (max_turns + 1u) <= (1ull << 16)) ? n * (max_turns + 1u) : 0;
    const size_t words = sizeof(ge_rollout_stats) / 8;
    void *pl = nullptr, *sp = nullptr, *ev = nullptr, *vw = nullptr, *fs = nullptr;
    napi_value pbuf, sbuf, ebuf, vbuf, fbuf, parr, sarr, farr, out;
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(uint32_t), &pl, &pbuf));
    NAPI_OK(napi_create_arraybuffer(env, n * sizeof(uint32_t), &sp, &sbuf));
    NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(ge_turn_event), &ev, &ebuf));
    NAPI_OK(napi_create_arraybuffer(env, slots * sizeof(ge_room_view), &vw, &vbuf));
    NAPI_OK(napi_create_arraybuffer(env, points * sizeof(ge_rollout_stats), &fs, &fbuf));
    // an empty list: N-API may give no data pointer for an empty buffer, and the library refuses forecast_keys or stats NULL before
    // it answers n == 0 - neither is read or written then
    static const uint64_t no_keys = 0;
    static ge_rollout_stats no_stats;
    if (!data[3]) data[3] = const_cast<uint64_t *>(&no_keys);
    if (!fs) fs = &no_stats;
    const int st = ge_batch_run_rooms_forecast(b, n, static_cast<const uint64_t *>(data[0]), static_cast<const uint64_t *>(data[1]),
                                               static_cast<const uint32_t *>(data[2]), max_turns, until, static_cast<const uint64_t *>(data[3]),
                                               static_cast<const uint32_t *>(data[4]), n_rollouts, pmax, seed, static_cast<uint32_t *>(pl),
                                               static_cast<uint32_t *>(sp), static_cast<ge_turn_event *>(ev),
                                               slots ? static_cast<ge_room_view *>(vw) : nullptr, slots * sizeof(ge_room_view),
                                               static_cast<ge_rollout_stats *>(fs), points * sizeof(ge_rollout_stats));
    if (st != GE_OK) return throw_status(env, st, "runRoomsForecast");
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, pbuf, 0, &parr));
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, sbuf, 0, &sarr));
    NAPI_OK(napi_create_typedarray(env, napi_biguint64_array, points * words, fbuf, 0, &farr));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "played", parr));
    NAPI_OK(napi_set_named_property(env, out, "stopped", sarr));
    NAPI_OK(napi_set_named_property(env, out, "events", ebuf));
    NAPI_OK(napi_set_named_property(env, out, "views", vbuf));
    NAPI_OK(napi_set_named_property(env, out, "stats", farr));
    return out;
}

bool is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

// rollout(batch, rooms: BigUint64Array, keys: BigUint64Array, turns: Uint32Array, seats: Uint32Array | null, firstAction: Uint32Array
// (rooms.length + 1) | null, playerIds: Uint32Array | null, choices: Uint32Array | null, nRollouts, maxTurns, seed: bigint):
// { words: BigUint64Array of rooms.length x 77 (ge_rollout_stats k at [77 k, 77 k + 77)), status: Int32Array of rooms.length } -
// index.js's rolloutRooms / rolloutActions / rolloutSeats: ge_batch_rollout_seats with seats, else ge_batch_rollout_actions with
// actions, else ge_batch_rollout_rooms.  A refused entry's words are 0 and its status < 0.  Two more arguments, baseline and
// subjects (Uint32Array of rooms.length each, with seats): index.js's rolloutCompare, ge_batch_rollout_compare; the result gains
// cmp: BigUint64Array of rooms.length x 6 (ge_compare_stats k at [6 k, 6 k + 6)).  One more, beliefs (Uint8Array of rooms.length x
// GE_BELIEF_SLOTS, with seats): index.js's rolloutBeliefs, ge_batch_rollout_beliefs - with or without baseline and subjects
napi_value Rollout(napi_env env, napi_callback_info info) {
    size_t argc = 14;
    napi_value argv[14];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    const bool seats = argc > 4 && !is_nullish(env, argv[4]), acts = argc > 5 && !is_nullish(env, argv[5]);
    const bool compare = argc > 12 && !is_nullish(env, argv[11]) && !is_nullish(env, argv[12]);
    const bool weighted = argc > 13 && !is_nullish(env, argv[13]);
    const char *what = weighted ? "rolloutBeliefs" : compare ? "rolloutCompare" : seats ? "rolloutSeats" : acts ? "rolloutActions" : "rolloutRooms";
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 11) return throw_status(env, GE_ERR_ARG, what);
    // rooms, keys, turns, then seats and firstAction, playerIds, choices where given
    napi_typedarray_type tt[7] = {};
    size_t len[7] = {0};
    void *data[7] = {nullptr};
    for (int k = 0; k < 7; k++) {
        if ((k == 3 && !seats) || (k > 3 && !acts)) continue;
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[1 + k], &tt[k], &len[k], &data[k], &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, what, "typed arrays expected");
    }
    const bool shape = tt[0] == napi_biguint64_array && tt[1] == napi_biguint64_array && tt[2] == napi_uint32_array && len[0] == len[1] &&
                       len[1] == len[2] && (!seats || (tt[3] == napi_uint32_array && len[3] == len[0])) &&
                       (!acts || (tt[4] == napi_uint32_array && tt[5] == napi_uint32_array && tt[6] == napi_uint32_array &&
                                  len[4] == len[0] + 1 && len[5] == len[6] && static_cast<const uint32_t *>(data[4])[len[0]] == len[5]));
    if (!shape)
        return throw_status(env, GE_ERR_ARG, what,
                            !seats && !acts ? "BigUint64Array, BigUint64Array, Uint32Array of equal length"
                            : seats ? "BigUint64Array x 2, Uint32Array (turns, seats) of equal length; Uint32Array offsets (length + 1) ending "
                                      "at the length of the Uint32Array players and choices"
                                    : "BigUint64Array x 2, Uint32Array (turns) of equal length; Uint32Array offsets (length + 1) ending at the "
                                      "length of the Uint32Array players and choices");
    const uint32_t *base = nullptr, *subj = nullptr;
    if (compare) {
        napi_typedarray_type ct[2];
        size_t cl[2];
        void *cd[2];
        for (int k = 0; k < 2; k++) {
            napi_value ab;
            size_t off;
            if (napi_get_typedarray_info(env, argv[11 + k], &ct[k], &cl[k], &cd[k], &ab, &off) != napi_ok)
                return throw_status(env, GE_ERR_ARG, what, "typed arrays expected");
        }
        if (!seats || ct[0] != napi_uint32_array || ct[1] != napi_uint32_array || cl[0] != len[0] || cl[1] != len[0])
            return throw_status(env, GE_ERR_ARG, what, "seats, baseline, subjects: Uint32Array of the entries' length");
        base = static_cast<const uint32_t *>(cd[0]);
        subj = static_cast<const uint32_t *>(cd[1]);
    }
    const uint8_t *beliefs = nullptr;
    if (weighted) {
        napi_typedarray_type bt;
        size_t bl;
        void *bd;
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, argv[13], &bt, &bl, &bd, &ab, &off) != napi_ok)
            return throw_status(env, GE_ERR_ARG, what, "typed arrays expected");
        const bool partial = argc > 12 && (is_nullish(env, argv[11]) != is_nullish(env, argv[12]));
        if (!seats || partial || bt != napi_uint8_array || bl != len[0] * GE_BELIEF_SLOTS)
            return throw_status(env, GE_ERR_ARG, what, "seats; beliefs: Uint8Array of 16 bytes per entry; baseline and subjects together or neither");
        beliefs = static_cast<const uint8_t *>(bd);
    }
    uint32_t n_rollouts = 0, max_turns = 0;
    uint64_t seed = 0;
    if (napi_get_value_uint32(env, argv[8], &n_rollouts) != napi_ok || napi_get_value_uint32(env, argv[9], &max_turns) != napi_ok ||
        !get_u64(env, argv[10], &seed))
        return throw_status(env, GE_ERR_ARG, what, "nRollouts, maxTurns: numbers; seed: bigint");
    void *cmp_data = nullptr;
    napi_value cmp_buf, cmp_arr;
    if (compare) {
        NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(ge_compare_stats), &cmp_data, &cmp_buf));
        memset(cmp_data, 0, len[0] * sizeof(ge_compare_stats));
    }
    const size_t words = sizeof(ge_rollout_stats) / 8;
    void *out = nullptr, *st_data = nullptr;
    napi_value buf, arr, st_buf, st_arr, res;
    NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(ge_rollout_stats), &out, &buf));
    memset(out, 0, len[0] * sizeof(ge_rollout_stats));
    NAPI_OK(napi_create_arraybuffer(env, len[0] * sizeof(int32_t), &st_data, &st_buf));
    int32_t *status = static_cast<int32_t *>(st_data);
    for (size_t k = 0; k < len[0]; k++) status[k] = 1;           // 1: untouched (no ge_status is positive)
    const uint64_t *rooms = static_cast<const uint64_t *>(data[0]), *keys = static_cast<const uint64_t *>(data[1]);
    const uint32_t *turns = static_cast<const uint32_t *>(data[2]), *sv = static_cast<const uint32_t *>(data[3]);
    const uint32_t *first = static_cast<const uint32_t *>(data[4]), *pl = static_cast<const uint32_t *>(data[5]);
    const uint32_t *ch = static_cast<const uint32_t *>(data[6]);
    ge_rollout_stats *o = static_cast<ge_rollout_stats *>(out);
    const int st = weighted ? ge_batch_rollout_beliefs(b, len[0], rooms, keys, turns, sv, first, pl, ch, status, beliefs, n_rollouts, max_turns,
                                                       seed, o, base, subj, static_cast<ge_compare_stats *>(cmp_data))
                   : compare ? ge_batch_rollout_compare(b, len[0], rooms, keys, turns, sv, first, pl, ch, status, n_rollouts, max_turns, seed, o,
                                                      base, subj, static_cast<ge_compare_stats *>(cmp_data))
                   : seats ? ge_batch_rollout_seats(b, len[0], rooms, keys, turns, sv, first, pl, ch, status, n_rollouts, max_turns, seed, o)
                   : acts ? ge_batch_rollout_actions(b, len[0], rooms, keys, turns, first, pl, ch, status, n_rollouts, max_turns, seed, o)
                          : ge_batch_rollout_rooms(b, len[0], rooms, keys, turns, n_rollouts, max_turns, seed, o);
    if (st != GE_OK) {
        // a refused entry returns its status with every verdict written; a structural error or a failure of the call leaves
        // the verdicts untouched (ge_batch_rollout_rooms writes none)
        bool untouched = false;
        for (size_t k = 0; k < len[0] && !untouched; k++) untouched = status[k] == 1;
        if (untouched) return throw_status(env, st, what);
    }
    NAPI_OK(napi_create_typedarray(env, napi_biguint64_array, len[0] * words, buf, 0, &arr));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, len[0], st_buf, 0, &st_arr));
    NAPI_OK(napi_create_object(env, &res));
    NAPI_OK(napi_set_named_property(env, res, "words", arr));
    NAPI_OK(napi_set_named_property(env, res, "status", st_arr));
    if (compare) {
        NAPI_OK(napi_create_typedarray(env, napi_biguint64_array, len[0] * (sizeof(ge_compare_stats) / 8), cmp_buf, 0, &cmp_arr));
        NAPI_OK(napi_set_named_property(env, res, "cmp", cmp_arr));
    }
    return res;
}

// readRoomsAt(batch, rooms: BigUint64Array): ArrayBuffer of rooms.length ge_room_view, view k = room rooms[k]
napi_value ReadRoomsAt(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 2) return throw_status(env, GE_ERR_ARG, "readRoomsAt");
    napi_typedarray_type tt;
    size_t len, off;
    void *rooms = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &tt, &len, &rooms, &ab, &off) != napi_ok || tt != napi_biguint64_array)
        return throw_status(env, GE_ERR_ARG, "readRoomsAt", "BigUint64Array expected");
    void *data = nullptr;
    napi_value buf;
    NAPI_OK(napi_create_arraybuffer(env, len * sizeof(ge_room_view), &data, &buf));
    int st = ge_batch_read_rooms_at(b, len, static_cast<const uint64_t *>(rooms), static_cast<ge_room_view *>(data), len * sizeof(ge_room_view));
    if (st != GE_OK) return throw_status(env, st, "readRoomsAt");
    return buf;
}

// writeRoomsAt(batch, rooms: BigUint64Array, views: ArrayBuffer of rooms.length ge_room_view): view k -> room rooms[k], all or nothing
napi_value WriteRoomsAt(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b || argc < 3) return throw_status(env, GE_ERR_ARG, "writeRoomsAt");
    napi_typedarray_type tt;
    size_t len, off, bytes = 0;
    void *rooms = nullptr, *data = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &tt, &len, &rooms, &ab, &off) != napi_ok || tt != napi_biguint64_array ||
        napi_get_arraybuffer_info(env, argv[2], &data, &bytes) != napi_ok || bytes != len * sizeof(ge_room_view))
        return throw_status(env, GE_ERR_ARG, "writeRoomsAt", "BigUint64Array and an ArrayBuffer of as many room views");
    const int st = ge_batch_write_rooms_at(b, len, static_cast<const uint64_t *>(rooms), static_cast<const ge_room_view *>(data));
    if (st == GE_ERR_ARG && len) {                // all-or-nothing: say which room's view did not fit its segment, if one did not
        const uint64_t bad = ge_last_rejected_room();
        for (size_t k = 0; k < len; k++)
            if (static_cast<const uint64_t *>(rooms)[k] == bad) {
                const std::string d = "room " + std::to_string(bad) + " does not fit its segment (nothing was written)";
                return throw_status(env, st, "writeRoomsAt", d.c_str());
            }
    }
    if (st != GE_OK) return throw_status(env, st, "writeRoomsAt");
    return nullptr;
}

// summary(batch): BigUint64Array-compatible ArrayBuffer of ge_summary words
napi_value Summary(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b) return throw_status(env, GE_ERR_ARG, "summary");
    void *data = nullptr;
    napi_value buf;
    NAPI_OK(napi_create_arraybuffer(env, sizeof(ge_summary), &data, &buf));
    int st = ge_batch_summary(b, static_cast<ge_summary *>(data));
    if (st != GE_OK) return throw_status(env, st, "summary");
    return buf;
}

napi_value Reset(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_batch *b = argc >= 1 ? batch_arg(env, argv[0]) : nullptr;
    if (!b) return throw_status(env, GE_ERR_ARG, "reset");
    int st = ge_batch_reset(b);
    if (st != GE_OK) return throw_status(env, st, "reset");
    return nullptr;
}

napi_value DeviceCount(napi_env env, napi_callback_info) {
    napi_value v;
    NAPI_OK(napi_create_int32(env, ge_device_count(), &v));
    return v;
}

napi_value RoomViewSize(napi_env env, napi_callback_info) {
    napi_value v;
    NAPI_OK(napi_create_int32(env, (int32_t)sizeof(ge_room_view), &v));
    return v;
}

// ---- device group: ONE Node process, N GPUs (ge_group_*, include/ge_step.h): rooms sharded over the devices, stepped
// concurrently, one RCCL all-gather of the per-device summaries inside the native library
struct GroupBox {
    ge_group *g = nullptr;
    bool busy = false;
};
void finalize_group(napi_env, void *data, void *) {
    GroupBox *box = static_cast<GroupBox *>(data);
    if (box->g) ge_group_destroy(box->g);
    delete box;
}
GroupBox *group_box(napi_env env, napi_value v) {
    GroupBox *box = nullptr;
    if (napi_get_value_external(env, v, reinterpret_cast<void **>(&box)) != napi_ok) return nullptr;
    return box;
}
ge_group *group_arg(napi_env env, napi_value v) {
    GroupBox *box = group_box(env, v);
    if (!box || !box->g) return nullptr;
    if (box->busy) {
        napi_throw_error(env, "GE_BUSY", "an async step() of this group is in flight: await it first (a ge_group handle is not thread-safe)");
        return nullptr;
    }
    return box->g;
}

// createGroup({seed, firstRoom, maxFuse, restart, trace, segments (the WHOLE job), devices: [0, 1, ...]}): External<ge_group>
napi_value CreateGroup(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 1) return throw_status(env, GE_ERR_ARG, "createGroup");
    ge_batch_desc d;
    if (!parse_desc(env, argv[0], "createGroup", &d)) return nullptr;
    napi_value devs;
    uint32_t n = 0;
    bool is_arr = false;
    if (napi_get_named_property(env, argv[0], "devices", &devs) != napi_ok || napi_is_array(env, devs, &is_arr) != napi_ok || !is_arr ||
        napi_get_array_length(env, devs, &n) != napi_ok || n == 0 || n > 64)
        return throw_status(env, GE_ERR_ARG, "createGroup", "devices");
    std::vector<int> devices(n);
    for (uint32_t i = 0; i < n; i++) {
        napi_value v;
        uint64_t x = 0;
        if (napi_get_element(env, devs, i, &v) != napi_ok || !get_u64(env, v, &x)) return throw_status(env, GE_ERR_ARG, "createGroup", "devices");
        devices[i] = (int)x;
    }
    ge_group *g = nullptr;
    int st = ge_group_create(&d, devices.data(), (int)n, &g);
    if (st != GE_OK) return throw_status(env, st, "createGroup");
    GroupBox *box = new GroupBox();
    box->g = g;
    napi_value ext;
    if (napi_create_external(env, box, finalize_group, nullptr, &ext) != napi_ok) {
        ge_group_destroy(g);
        delete box;
        napi_throw_error(env, "GE_NAPI", "napi_create_external failed");
        return nullptr;
    }
    return ext;
}

struct GroupStepWork {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref keep;
    GroupBox *box;
    uint32_t turns;
    int status;
};
void group_step_execute(napi_env, void *data) {
    GroupStepWork *w = static_cast<GroupStepWork *>(data);
    w->status = ge_group_step(w->box->g, w->turns);            // all devices step concurrently
    if (w->status == GE_OK) w->status = ge_group_sync(w->box->g);
}
void group_step_complete(napi_env env, napi_status, void *data) {
    GroupStepWork *w = static_cast<GroupStepWork *>(data);
    w->box->busy = false;
    napi_value v;
    if (w->status == GE_OK) {
        napi_get_undefined(env, &v);
        napi_resolve_deferred(env, w->deferred, v);
    } else {
        napi_value msg;
        napi_create_string_utf8(env, ge_strerror(w->status), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &v);
        napi_reject_deferred(env, w->deferred, v);
    }
    napi_delete_async_work(env, w->work);
    napi_delete_reference(env, w->keep);
    delete w;
}

// groupStep(group, nTurns): Promise<void> - on the libuv pool, like step()
napi_value GroupStep(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_group *g = argc >= 1 ? group_arg(env, argv[0]) : nullptr;
    uint64_t turns = 1;
    if (!g || (argc > 1 && !get_u64(env, argv[1], &turns))) return throw_status(env, GE_ERR_ARG, "groupStep");
    GroupStepWork *w = new GroupStepWork();
    w->box = group_box(env, argv[0]); w->turns = (uint32_t)turns; w->status = GE_OK;
    napi_value promise, name;
    if (napi_create_reference(env, argv[0], 1, &w->keep) != napi_ok) { delete w; return throw_status(env, GE_ERR_ARG, "groupStep"); }
    if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
        napi_create_string_utf8(env, "ge_group_step", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_async_work(env, nullptr, name, group_step_execute, group_step_complete, w, &w->work) != napi_ok) {
        napi_delete_reference(env, w->keep);
        delete w;
        return throw_status(env, GE_ERR_ARG, "groupStep");
    }
    w->box->busy = true;
    if (napi_queue_async_work(env, w->work) != napi_ok) {
        w->box->busy = false;
        napi_delete_async_work(env, w->work);
        napi_delete_reference(env, w->keep);
        delete w;
        return throw_status(env, GE_ERR_ARG, "groupStep");
    }
    return promise;
}

// groupSummary(group): ArrayBuffer holding the whole job's ge_summary (per-device reductions + ONE ncclAllGather + sum)
napi_value GroupSummary(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_group *g = argc >= 1 ? group_arg(env, argv[0]) : nullptr;
    if (!g) return throw_status(env, GE_ERR_ARG, "groupSummary");
    void *data = nullptr;
    napi_value buf;
    NAPI_OK(napi_create_arraybuffer(env, sizeof(ge_summary), &data, &buf));
    int st = ge_group_summary(g, static_cast<ge_summary *>(data));
    if (st != GE_OK) return throw_status(env, st, "groupSummary");
    return buf;
}

// groupReadRooms(group, shard, first, count): ArrayBuffer of ge_room_view from device `shard`'s batch (local indices)
napi_value GroupReadRooms(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    ge_group *g = argc >= 1 ? group_arg(env, argv[0]) : nullptr;
    uint64_t shard = 0, first = 0, count = 0;
    if (!g || argc < 4 || !get_u64(env, argv[1], &shard) || !get_u64(env, argv[2], &first) || !get_u64(env, argv[3], &count))
        return throw_status(env, GE_ERR_ARG, "groupReadRooms");
    ge_batch *b = nullptr;
    int st = ge_group_shard(g, (int)shard, &b);
    if (st != GE_OK) return throw_status(env, st, "groupReadRooms");
    void *data = nullptr;
    napi_value buf;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)count * sizeof(ge_room_view), &data, &buf));
    st = ge_batch_read_rooms(b, first, count, static_cast<ge_room_view *>(data), (size_t)count * sizeof(ge_room_view));
    if (st != GE_OK) return throw_status(env, st, "groupReadRooms");
    return buf;
}

napi_value DestroyGroup(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    GroupBox *box = argc >= 1 ? group_box(env, argv[0]) : nullptr;
    if (!box) return throw_status(env, GE_ERR_ARG, "destroyGroup");
    if (box->busy) { napi_throw_error(env, "GE_BUSY", "destroyGroup while an async step() is in flight"); return nullptr; }
    if (box->g) { ge_group_destroy(box->g); box->g = nullptr; }
    return nullptr;
}

napi_value Init(napi_env env, napi_value exports) {
    napi_property_descriptor props[] = {
        {"compileTable", nullptr, CompileTable, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"tableInfo", nullptr, TableInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"createBatch", nullptr, CreateBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"step", nullptr, Step, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"stepSync", nullptr, StepSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"readRooms", nullptr, ReadRooms, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"injectAction", nullptr, InjectAction, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"injectActions", nullptr, InjectActions, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"setTurn", nullptr, SetTurn, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"writeRooms", nullptr, WriteRooms, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"destroyBatch", nullptr, DestroyBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"readEvents", nullptr, ReadEvents, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"stepRooms", nullptr, StepRooms, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"stepRoomsPlayout", nullptr, StepRoomsPlayout, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"runRooms", nullptr, RunRooms, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"runRoomsPlayout", nullptr, RunRoomsPlayout, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"runRoomsForecast", nullptr, RunRoomsForecast, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"findRooms", nullptr, FindRooms, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"setSeats", nullptr, SetSeats, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"adviseSeats", nullptr, AdviseSeats, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"seats", nullptr, Seats, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"clearSeats", nullptr, ClearSeats, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"readRoomsAt", nullptr, ReadRoomsAt, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"rollout", nullptr, Rollout, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"writeRoomsAt", nullptr, WriteRoomsAt, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"summary", nullptr, Summary, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"reset", nullptr, Reset, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"roomViewSize", nullptr, RoomViewSize, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"createGroup", nullptr, CreateGroup, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"groupStep", nullptr, GroupStep, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"groupSummary", nullptr, GroupSummary, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"groupReadRooms", nullptr, GroupReadRooms, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"destroyGroup", nullptr, DestroyGroup, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
