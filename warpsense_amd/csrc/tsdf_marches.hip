// tsdf_marches.hip — the translation unit of tsdf_tail.hip and tsdf_free.hip: one file per march for the reader, one unit for the
// compiler.  (tsdf_setup.hip and tsdf_resolve.hip are units of their own.)
//
// The two are compiled together because the compiler does not keep the tail march the same without the free pass.  Measured with
// tools/device_code_diff.py --by-kernel against the single file all four stages came from, same text, same flags:
//   tsdf_setup.hip alone, tsdf_free.hip alone, tsdf_resolve.hip alone   every kernel the same code
//   tsdf_tail.hip alone                     march_tail_kernel<false> comes out different (same arithmetic, other registers, another order;
//                                           the first difference lies where a voxel byte's 64-bit address is formed); <true> the same
//   tsdf_tail.hip + tsdf_setup.hip          march_tail_kernel<false> different
//   tsdf_tail.hip + tsdf_resolve.hip        march_tail_kernel<false> different
//   tsdf_tail.hip + tsdf_free.hip           all four march kernels the same code, in either order (also with tsdf_setup.hip, and with all four)
// The layout below was then compared as a whole library, with the default flags, with the three timing switches and with
// -DWS_TAIL_KO=31 -DWS_RESOLVE_KO=7: profiles/tsdf_split.json.  Why the tail march needs the free pass was not traced; reg_routes.hip has
// a reading of the same effect for the registration kernels.
// Whoever separates these files, or gives a helper of tsdf_scatter.h / tsdf_pool.h another caller, compares the kernels again: their
// instructions can change without a change to their text.
#include "tsdf_tail.hip"
#include "tsdf_free.hip"
