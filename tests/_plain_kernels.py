"""The plain device kernels -- every __global__ kernel of the build that tests/_kernel_matrix.py does not claim (kernel_of_symbol,
pbdiag_of_symbol) -- as a table: where each is defined, how it is launched, how many items one grid covers where the launcher caps the
grid, and which GPU test runs it past that size (tests/test_plain_kernel_inventory.py holds the table against the build, the sources and
the test modules on the CPU; no tests in here).

Most of these kernels are launched on a CAPPED grid and reach everything beyond it with a stride loop.  A wrong stride, an accumulator
that survives into the second lap or a counter dropped between laps shows only when a launch holds more items than one grid covers, so
every capped kernel names a test whose largest stated size exceeds one grid.  The caps are restated here as data, each with the file and
the exact expression it restates (as _fused_rounds.py restates the fused launcher's grid): a changed cap is a changed table."""
import re
from collections import namedtuple

CSRC = "ceedpetscsolid_amd/csrc/"

# ---------------------------------------------------------------------------------------------------------------------------------
# the caps: launch form -> (file, the expressions restated -- each must stand verbatim in the file --, items one grid covers)
# ---------------------------------------------------------------------------------------------------------------------------------
Cap = namedtuple("Cap", "file exprs items what")
CAPS = {
    "stream": Cap(CSRC + "kernels_common.hpp", ("size_t b = (n + 255) / 256;", "return dim3((unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)));",
                                                "hipLaunchKernelGGL(k, stream_grid(n), dim3(256), 0, s, args...);"),
                  2048 * 256, "launch_stream / stream_grid: min(2048, ceil(n / 256)) workgroups of 256 lanes, an item per lane and lap"),
    "grid_for": Cap(CSRC + "kernels_csr.hip", ("size_t b = (n + per_block - 1) / per_block;", "return dim3((unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b)));"),
                    4096 * 256, "grid_for(n, 256): min(4096, ceil(n / 256)) workgroups of 256 lanes"),
    "assemble unpack": Cap(CSRC + "kernels_assemble.hip", ("constexpr int AB = 256;", "const unsigned nb_un = (unsigned)std::min((nun + AB - 1) / AB, 1024);"),
                           1024 * 256, "k_assemble's extra workgroups nb_un: the arrivals of a halo exchange; its row workgroups are not capped"),
    "assemble_epi interior": Cap(CSRC + "kernels_assemble.hip",
                                 ("constexpr int AB = 256;", "const unsigned nb_int = (unsigned)std::min<size_t>(((size_t)std::max(ep.n_int, 0) * 3 + AB - 1) / AB, 4096);"),
                                 4096 * 256, "k_assemble_epi's extra workgroups nb_int: the dofs of the element-interior nodes; its row workgroups are not capped"),
    "spgemm dense": Cap(CSRC + "kernels_csr.hip", ("dim3((unsigned)std::min(nrows, 8192)), dim3(64)",), 8192, "a one-wave workgroup per row of C, at most 8192"),
    "spgemm row": Cap(CSRC + "kernels_csr.hip", ("dim3((unsigned)std::min(nrows, 32768)), dim3(64)",), 32768, "a one-wave workgroup per row of C, at most 32768"),
    "spgemm plain": Cap(CSRC + "kernels_csr.hip", ("const unsigned blocks = (unsigned)std::min<size_t>(((size_t)nrows + 3) / 4, 16384);",), 16384 * 4,
                        "a wave per row of C, four to a workgroup, at most 16384 workgroups"),
    "block gram": Cap(CSRC + "kernels_block.hip", ("const int grid = (int)(nchunks < (size_t)BLOCK_GRAM_MAX_PARTS ? nchunks : (size_t)BLOCK_GRAM_MAX_PARTS);",
                                                   "static_assert(4 * BG_R == 256"), 1024 * 64, "a chunk of BLOCK_GRAM_ROWS = 64 rows per workgroup and lap, at most BLOCK_GRAM_MAX_PARTS"),
    "block combine": Cap(CSRC + "kernels_block.hip", ("const dim3 g((unsigned)(nchunks < (size_t)BLOCK_COMBINE_MAX_GROUPS ? nchunks : (size_t)BLOCK_COMBINE_MAX_GROUPS)), b(256);",),
                         2048 * 512, "a chunk of BLOCK_COMBINE_ROWS = 512 rows per workgroup and lap, at most BLOCK_COMBINE_MAX_GROUPS"),
}
# constants the items above are products of, where the expression names them: (file, the definition verbatim)
CAP_CONSTANTS = [(CSRC + "kernels.hpp", "constexpr int BLOCK_GRAM_MAX_PARTS = 1024;"), (CSRC + "kernels.hpp", "constexpr int BLOCK_COMBINE_ROWS = 512;"),
                 (CSRC + "kernels.hpp", "constexpr int BLOCK_COMBINE_MAX_GROUPS = 2048;"), (CSRC + "kernels_block.hip", "constexpr int BG_R = BLOCK_GRAM_ROWS;")]
UNCAPPED = ("one workgroup per unit", "single workgroup", "persistent groups")     # launch forms without a cap of their own

STREAM_ITEMS = CAPS["stream"].items
GRID_FOR_ITEMS = CAPS["grid_for"].items


def lap_sizes(G):
    """The sizes at which a kernel whose grid covers G items is run: one short of a grid, a whole grid, one item into the second lap,
    and two laps and three items (some lanes take three)."""
    return [G - 1, G, G + 1, 2 * G + 3]


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
# tests: node ids "module::function" of GPU tests.  sizes: where the largest size of those tests is stated --
#   ("attr", module, name)               a module-level int or sequence of ints of the test module, imported as data;
#   ("text", file, snippet, value)       a literal inside a test body: the snippet must stand verbatim in the file, `value` restates it.
# reach: for a cap no caller can reach -- (largest item count the entry points let through, [(file, expression verbatim), ..] that
# limit it); such a kernel names the test of its largest reachable size and the test that pins the limit.
Kernel = namedtuple("Kernel", "name file launch tests sizes reach note", defaults=(None, None, ""))
LAPS, LIN, AMG, BLK = "test_grid_laps_gpu", "test_linalg_kernels", "test_amg", "test_block_vectors_gpu"


def _k(name, file, launch, tests, sizes=None, reach=None, note=""):
    return Kernel(name, CSRC + file, launch, tuple(tests), sizes, reach, note)


KERNELS = [
    # ---- kernels_assemble.hip
    _k("k_rstr", "kernels_assemble.hip", "stream", [f"{LAPS}::test_restriction_around_one_grid", f"{LAPS}::test_restriction_on_the_degree7_box"], ("attr", LAPS, "STREAM_SIZES"),
       note="items: entries of the E-vector"),
    _k("k_rstr_transpose", "kernels_assemble.hip", "stream", [f"{LAPS}::test_restriction_around_one_grid", f"{LAPS}::test_restriction_on_the_degree7_box"],
       ("attr", LAPS, "STREAM_SIZES"), note="items: rows of the transpose map x components"),
    _k("k_multiplicity", "kernels_assemble.hip", "stream", [f"{LAPS}::test_restriction_around_one_grid", f"{LAPS}::test_restriction_on_the_degree7_box"],
       ("attr", LAPS, "STREAM_SIZES"), note="items: rows of the transpose map x components"),
    _k("k_assemble", "kernels_assemble.hip", "assemble unpack", [f"{LAPS}::test_folded_halo_on_the_degree7_box"], ("attr", LAPS, "FOLDED_HALO_SIZES"),
       note="items: distinct destinations of the arrivals"),
    _k("k_assemble_epi", "kernels_assemble.hip", "assemble_epi interior", [f"{LAPS}::test_fused_epilogue_on_the_degree7_box"], ("attr", LAPS, "BOX7_INTERIOR_DOFS"),
       note="items: dofs of the element-interior nodes; the fused forms always sum in one segment (launch_info), under the serial and the default form alike"),
    _k("k_halo_pack", "kernels_assemble.hip", "stream", [f"{LAPS}::test_halo_exchange_around_one_grid"], ("attr", LAPS, "STREAM_SIZES"), note="items: entries of all lists"),
    _k("k_halo_unpack_add", "kernels_assemble.hip", "stream", [f"{LAPS}::test_halo_exchange_around_one_grid"], ("attr", LAPS, "STREAM_SIZES"),
       note="items: distinct destinations"),
    # ---- kernels_block.hip
    _k("k_block_gram", "kernels_block.hip", "block gram", [f"{BLK}::test_gram_past_a_full_grid_of_partials"],
       ("text", "tests/test_block_vectors_gpu.py", "check_gram(gpu, 3 * pmax * R - 5, 3, 5, pads=(0,), a0=0, b0=0)", 3 * 1024 * 64 - 5), note="items: rows"),
    _k("k_block_gram_final", "kernels_block.hip", "one workgroup per unit", [f"{BLK}::test_gram_rows_and_columns"], note="64 entries of G per workgroup"),
    _k("k_block_combine", "kernels_block.hip", "block combine", [f"{BLK}::test_combine_past_a_full_grid"],
       ("text", "tests/test_block_vectors_gpu.py", "check_combine(gpu, groups * rows + 1, 1, 1, pads=(1,), a0=0, y0=0)", 2048 * 512 + 1), note="items: rows"),
    # ---- kernels_contact.hip, kernels_surface.hip
    _k("k_contact", "kernels_contact.hip", "one workgroup per unit", ["test_contact_gpu::test_every_instantiation_against_the_portable_form"], note="faces, FPW to a wave"),
    _k("k_surface", "kernels_surface.hip", "one workgroup per unit", ["test_surface_load_gpu::test_every_instantiation_against_the_portable_form"], note="faces, FPW to a wave"),
    _k("k_surface_sum", "kernels_surface.hip", "stream", [f"{LAPS}::test_surface_loads_on_a_sheet_past_one_grid", f"{LAPS}::test_contact_on_a_sheet_past_one_grid"],
       ("attr", LAPS, "SHEET_ROWS"), note="items: face-node rows; the bottom of box_mesh(362, 362, 1) at degree 2, whose dofmap takes about four seconds to build"),
    # ---- kernels_coord.hip
    _k("k_coord_op", "kernels_coord.hip", "one workgroup per unit", ["test_coord_energy_gpu::test_true_solution_and_diagnostics_at_every_P"], note="an element per workgroup"),
    _k("k_energy_op", "kernels_coord.hip", "one workgroup per unit", ["test_coord_energy_gpu::test_strain_energy_and_forcing_at_every_P_and_Q"], note="an element per workgroup"),
    # ---- kernels_csr.hip
    _k("k_csr_sum", "kernels_csr.hip", "grid_for", [f"{LAPS}::test_csr_assembly_around_one_grid"], ("attr", LAPS, "GRID_FOR_SIZES"), note="items: entries of the pattern"),
    _k("k_csr_unit_diag", "kernels_csr.hip", "grid_for", [f"{LAPS}::test_csr_assembly_around_one_grid"], ("attr", LAPS, "GRID_FOR_SIZES"), note="items: unit rows"),
    _k("k_csr_diag", "kernels_csr.hip", "grid_for", [f"{LAPS}::test_csr_assembly_around_one_grid"], ("attr", LAPS, "GRID_FOR_SIZES"), note="items: rows"),
    _k("k_csr_spmv_stream", "kernels_csr.hip", "one workgroup per unit", [f"{LIN}::test_spmv_shapes_on_device"], note="a run of rows per workgroup"),
    _k("k_csr_spgemm", "kernels_csr.hip", "spgemm plain", [f"{LAPS}::test_products_past_one_grid_of_rows"], ("attr", LAPS, "PLAIN_PRODUCT_ROWS"), note="items: rows of C"),
    _k("k_csr_spgemm_row", "kernels_csr.hip", "spgemm row", [f"{LAPS}::test_products_past_one_grid_of_rows"], ("attr", LAPS, "ROW_PRODUCT_ROWS"), note="items: rows of C"),
    _k("k_csr_spgemm_dense", "kernels_csr.hip", "spgemm dense", [f"{LIN}::test_dense_product_on_device", f"{LAPS}::test_a_dense_product_cannot_outgrow_its_grid"],
       ("text", "tests/test_linalg_kernels.py", '@pytest.mark.gpu\n@pytest.mark.parametrize("n", [4096, 4097])\ndef test_dense_product_on_device', 4096),
       reach=(4096, [(CSRC + "ceed_csr.cpp", 'if (dense && nrows != ncols) return ceed_error("CeedXCsrCreateProduct: a dense result must be square");'),
                     (CSRC + "kernels_csr.hip", "constexpr int CSR_DENSE_MAX_COLS = 4096;"),
                     (CSRC + "kernels_csr.hip", "if (dense_ncols > 0 && dense_ncols <= CSR_DENSE_MAX_COLS) {")]),
       note="items: rows of C.  A dense result is square and holds at most 4096 columns, so at most 4096 rows reach this kernel: its loop never takes a second lap"),
    _k("k_gj_pivot", "kernels_csr.hip", "single workgroup", [f"{AMG}::test_dense_inverse_on_device"]),
    _k("k_gj_panel", "kernels_csr.hip", "one workgroup per unit", [f"{AMG}::test_dense_inverse_on_device"], note="a 32 x 32 tile per workgroup; n = 33, 65, 70: ragged tiles"),
    _k("k_gj_update", "kernels_csr.hip", "one workgroup per unit", [f"{AMG}::test_dense_inverse_on_device"], note="a 32 x 32 tile per workgroup"),
    _k("k_symmetrize", "kernels_csr.hip", "grid_for", [f"{AMG}::test_dense_inverse_on_device"], ("attr", AMG, "DENSE_INVERSE_ENTRIES"), note="items: entries n x n of the matrix"),
    # ---- kernels_explicit.hip
    _k("k_leapfrog", "kernels_explicit.hip", "stream", ["test_explicit_gpu::test_entry_point_against_the_portable_form"], ("attr", "test_explicit_gpu", "SIZES")),
    _k("k_leapfrog_final", "kernels_explicit.hip", "single workgroup", ["test_explicit_gpu::test_entry_point_against_the_portable_form"]),
    # ---- kernel_fused_pencil.hpp (the entry with the mass term: the family of _kernel_matrix is the entry without)
    _k("k_fused_pencil_mass", "kernel_fused_pencil.hpp", "persistent groups", ["test_fused_rounds_gpu::test_rounds_match_the_oracle"],
       note="the fused launcher's grid and its rounds: tests/_fused_rounds.py"),
    # ---- kernels_geometry.hip
    _k("k_geo_coeffs", "kernels_geometry.hip", "one workgroup per unit", ["test_physics_edges_gpu::test_special_and_general_geometry_agree_across_the_branches"],
       note="256 (element, component) lanes per workgroup"),
    _k("k_geo_affine", "kernels_geometry.hip", "one workgroup per unit", ["test_physics_edges_gpu::test_special_and_general_geometry_agree_across_the_branches"],
       note="256 elements per workgroup"),
    _k("k_geo_swept", "kernels_geometry.hip", "one workgroup per unit", ["test_physics_edges_gpu::test_special_and_general_geometry_agree_across_the_branches"],
       note="256 elements per workgroup"),
    # ---- kernels_mass.hip, kernels_stress.hip
    _k("k_mass", "kernels_mass.hip", "one workgroup per unit", ["test_mass_gpu::test_apply_add_and_diagonal_against_the_portable_form"], note="EPB elements per workgroup"),
    _k("k_stress", "kernels_stress.hip", "one workgroup per unit", ["test_stress_gpu::test_sweep_against_the_portable_form"], note="EPB elements per workgroup"),
    # ---- kernels_pointblock.hip
    _k("k_pb_assemble", "kernels_pointblock.hip", "stream", [f"{LAPS}::test_pointblock_diagonal_on_the_degree7_box"], ("attr", LAPS, "BOX7_NODES"), note="items: nodes"),
    _k("k_pb_invert", "kernels_pointblock.hip", "stream", ["test_pointblock_gpu::test_block_kernels_against_numpy"], ("attr", "test_pointblock_gpu", "BLOCK_NODES"), note="items: nodes"),
    _k("k_pb_mult", "kernels_pointblock.hip", "stream", ["test_pointblock_gpu::test_block_kernels_against_numpy"], ("attr", "test_pointblock_gpu", "BLOCK_NODES"), note="items: nodes"),
    _k("k_pb_cheb_step", "kernels_pointblock.hip", "stream", ["test_pointblock_gpu::test_block_kernels_against_numpy"], ("attr", "test_pointblock_gpu", "BLOCK_NODES"),
       note="items: nodes"),
    # ---- kernels_transfer.hip
    _k("k_xfer_weights", "kernels_transfer.hip", "stream", [f"{LAPS}::test_transfer_weights_see_an_entry_beyond_one_grid"], ("attr", LAPS, "BOX7_LSIZE"), note="items: fine dofs"),
    # ---- kernels_vector.hip
    _k("k_set_value", "kernels_vector.hip", "stream", [f"{LIN}::test_set_value_on_device"], ("attr", LIN, "EDGE_SIZES")),
    _k("k_reciprocal", "kernels_vector.hip", "stream", [f"{LIN}::test_reciprocal_on_device"], ("attr", LIN, "EDGE_SIZES")),
    _k("k_pointwise_mult", "kernels_vector.hip", "stream", [f"{LIN}::test_elementwise_helpers_on_device"], ("attr", LIN, "ELEM_SIZES")),
    _k("k_axpby", "kernels_vector.hip", "stream", [f"{LIN}::test_elementwise_helpers_on_device"], ("attr", LIN, "ELEM_SIZES")),
    _k("k_waxpby", "kernels_vector.hip", "stream", [f"{LIN}::test_elementwise_helpers_on_device"], ("attr", LIN, "ELEM_SIZES")),
    _k("k_cheb_update", "kernels_vector.hip", "stream", [f"{LIN}::test_chebyshev_entries_on_device"], ("attr", LIN, "EDGE_SIZES")),
    _k("k_axpby_dev", "kernels_vector.hip", "stream", [f"{LIN}::test_axpby_scalars_on_device"], ("attr", LIN, "EDGE_SIZES")),
    _k("k_masked_copy", "kernels_vector.hip", "stream", [], reach=(0, []),
       note="launch_masked_copy is called by no entry point of the ABI: there is nothing to run it through (NO_CALLER: the check holds that none has appeared)"),
    _k("k_dot", "kernels_vector.hip", "stream", [f"{LIN}::test_dot_on_device"], ("attr", LIN, "DOT_SIZES"), note="its grid is stream_grid(n) itself"),
    _k("k_dot_final", "kernels_vector.hip", "single workgroup", [f"{LIN}::test_dot_on_device"]),
    _k("k_scalar_div", "kernels_vector.hip", "single workgroup", [f"{LIN}::test_scalar_divide_on_device"]),
    _k("k_clock_probe", "kernels_vector.hip", "single workgroup", [], note="one wave, one lane at work; launched by bench.py --full alone, no test runs it"),
]
BY_NAME = {k.name: k for k in KERNELS}
NO_CALLER = {"k_masked_copy": "launch_masked_copy"}      # kernel -> its launcher, which no .cpp file of csrc may name


def plain_name_of_symbol(mangled):
    """The kernel name of a mangled cps:: symbol (the first nested name after the namespace; template arguments dropped), or None for
    a symbol that is not of that namespace."""
    m = re.match(r"_ZN3cps(\d+)", mangled)
    if m is None:
        return None
    n = int(m[1])
    return mangled[m.end():m.end() + n]
