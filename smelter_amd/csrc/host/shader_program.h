// shader_program.h — a user shader program (include/smr.h "user shaders") as the two halves of the library see it: the host half
// (shader_program.cpp: the runtime compiler, the renderer's registry entries) owns the object, the device half (smr_user_shader.hip)
// hangs the loaded modules on it.  Plain C++: nothing here needs a HIP header.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "smr.h"

struct smr_shader_program {
    bool ok = false;           // compiled: `code` is a gfx950 code object
    std::string log;           // the compiler's messages (errors and warnings)
    std::vector<char> code;
    std::atomic<uint64_t> launches{0};

    // device half.  One module per device, loaded at the first launch there, shared by every context on that device (a renderer's
    // lanes), unloaded when the last of those contexts goes or with the program, whichever comes first.
    struct Module {
        int device = 0;
        void *module = nullptr, *function = nullptr;  // hipModule_t, hipFunction_t
        std::vector<smr_ctx *> users;
    };
    std::vector<Module> modules;                     // (guarded by the device half's lock)
    void (*unload)(smr_shader_program *) = nullptr;  // set by the device half with the first module: smr_shader_program_destroy calls it
};

// A registry entry of the renderer that is not a built-in id (renderer.cpp knows nothing else about user shaders: what it renders on —
// tests/san/null_device.cpp included — does not have to provide them).  `launch` is the twin of smr_builtin_shader; `release` (may be
// null) runs once when the entry is replaced or the renderer destroyed, after every context of the renderer has been synchronised.
struct smr_shader_hook {
    void *user = nullptr;
    int (*launch)(void *user, smr_ctx *ctx, const void *params, size_t params_size, const smr_surface *const *src, uint32_t n_src,
                  smr_surface *dst, float time_s) = nullptr;
    void (*release)(void *user) = nullptr;
};
int smr_renderer_register_shader_hook(smr_renderer *r, const char *shader_id, const smr_shader_hook &hook);  // renderer.cpp
int smr_renderer_fail(smr_renderer *r, int code, const std::string &msg);                                    // renderer.cpp
