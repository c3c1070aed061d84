// reg_routes.hip — the translation unit of reg_loop.hip, reg_launches.hip and reg_server.hip: one file per route for the reader, one
// unit for the compiler.  (reg_batch.hip is a unit of its own.)
//
// The three are compiled together because the compiler does not keep their kernels apart.  Measured with
// tools/device_code_diff.py --by-kernel against the single file they came from, same text, same flags:
//   reg_loop.hip alone                 reg_loop_kernel<*, false> come out different (same arithmetic, other registers, another order)
//   reg_server.hip alone               both reg_server_kernel
//   reg_server.hip + reg_launches.hip  reg_server_kernel<true>          (the same with reg_batch.hip in place of reg_launches.hip)
//   reg_server.hip + reg_loop.hip      reg_server_kernel<false> and reg_loop_kernel<*, false>
//   all three, in any order            every one of the eleven kernels the same code; reg_launches.hip and reg_batch.hip also alone
// What a kernel needs is the company of a kernel that calls the same helpers with OTHER arguments.  Every helper of the layers is
// __forceinline__, but a device function is internal to its unit and the interprocedural passes run before the inliner: where every
// caller of a unit passes the same constant -- the server's REG_STRIDE, per_group and `publish`, which the loop passes as variables;
// the `valid = true` and `cache = nullptr` of the points beyond the first two of a lane, which reg_iter_kernel and reg_pass_kernel
// pass otherwise -- the helper can be specialised first and inlined afterwards.  (That reading fits every row above; the passes
// themselves were not traced.)
// Whoever separates these files, or gives a helper a caller with other arguments, compares the kernels again: their instructions
// can change without a change to their text.
#include "reg_loop.hip"
#include "reg_launches.hip"
#include "reg_server.hip"
