"""Kernel-coverage record of the GPU test suite.

  on the GPU box:
      DIB_COVERAGE_LOG=/tmp/cov/tests.tsv rocprofv3 --kernel-trace --marker-trace -M -f csv -d /tmp/cov/trace -- \
          python -m pytest tests -m gpu -q
      python tools/kernel_coverage.py build /tmp/cov/trace /tmp/cov/tests.tsv gpurun_out/r06_suite_kernel_coverage.txt
  a suite too long for one visit is traced in parts (disjoint sets of test files, `build` once per part, anywhere afterwards):
      python tools/kernel_coverage.py merge profiles/r06_suite_kernel_coverage.txt PART_A.txt PART_B.txt
  anywhere (tests/test_kernel_coverage.py, no GPU):
      python tools/kernel_coverage.py check profiles/r06_suite_kernel_coverage.txt

`build` assigns every kernel dispatch of every traced process (pytest itself and the subprocesses its tests start) to the test
whose ROCTx range (tests/conftest.py) contains the dispatch's start timestamp, and writes, for every kernel symbol of
libdib_hip.so's gfx950 code object, the number of launches and the tests that launched it ('*' = the test compares with the
float64 / NumPy oracle, see ORACLE_TESTS).  `check` = every kernel symbol of the library as built here is on that list with at
least one test.
"""
import bisect
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "distributed-information-bottleneck.github.io_amd", "libdib_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# tests (file::function) whose assertions compare device results with an INDEPENDENT CPU checker: oracle/dib_oracle.py (float64
# NumPy), oracle/dib_torch_cpu.py (float64 autograd), the float64 loop / set-transformer oracles, plain NumPy float64 formulas
ORACLE_TESTS = {
    "test_gpu_parity.py": {
        "test_gemm_vs_numpy", "test_skinny_k_gemm_vs_numpy", "test_eps_matches_oracle_and_host_ref", "test_forward_backward_parity",
        "test_late_annealing_regime_small_sigma_large_mu", "test_split_batch_wgrad_and_dp_equivalence", "test_adam_matches_keras_form",
        "test_encode_deterministic_and_bhattacharyya", "test_fit_trajectory_matches_oracle_fit", "test_north_star_shape_properties",
        "test_mi_sandwich_bounds_match_oracle", "test_ib_flag_one_wide_feature_on_the_boolean_circuit",
        "test_infonce_loss_and_grads_match_oracle", "test_infonce_at_working_batch_sizes", "test_infonce_edge_shapes",
        "test_infonce_one_launch_path", "test_mi_sandwich_bounds_at_the_reference_evaluation_size", "test_dense_stack_matches_numpy",
        "test_dense_stack_row_tile_kernels", "test_autograd_bridge_matches_oracle_gradients",
        "test_hipgraph_fit_is_bit_identical_to_eager_and_matches_oracle", "test_north_star_architecture_multi_step_trajectory",
        "test_random_architectures_forward_backward"},
    "test_gpu_fullsize.py": {
        "test_config3_full_batch_step_all_gradients", "test_config3_full_batch_forward_against_an_independent_float64_forward", "test_config4_f50_full_batch_step_all_gradients",
        "test_config4_f50_ragged_batch_general_and_fused_paths_agree", "test_config3_fit_trajectory_beta_ramp_full_batch"},
    "test_gpu_set_transformer.py": {
        "test_forward_replays_the_notebook_fixture", "test_forward_backward_parity", "test_config5_size_4096_particles_flash_all_gradients",
        "test_config5_full_depth_six_blocks_at_4096_particles", "test_attention_backward_score_stash_equals_recompute",
        "test_train_steps_match_oracle_adam", "test_probe_grid_information_bounds_match_oracle",
        "test_backward_follows_the_forward_that_ran"},
    "test_gpu_trajectories.py": {
        "test_infonce_loop_trajectory_matches_float64_oracle", "test_keras_path_trajectory_160_steps_through_the_ramp"},
    "test_gpu_measurement.py": {
        "test_step_losses_and_all_gradients_match_oracle", "test_train_steps_through_the_beta_ramp_match_oracle_adam",
        "test_symbolize_matches_oracle", "test_mi_sandwich_bounds_of_the_ib_encoder_match_oracle"},
    "test_gpu_measurement_batched_kernels.py": {
        "test_measure_batched_equals_the_single_kernels_and_the_oracle",
        "test_infonce_batched_equals_the_single_entry_point_and_the_oracle", "test_infonce_batched_wide_embeddings"},
    "test_gpu_measurement_ensemble.py": {
        "test_step_losses_and_all_gradients_of_every_replica_match_oracle", "test_train_steps_through_the_beta_ramp_match_oracle_adam"},
    "test_gpu_circuit.py": {
        "test_drawn_rows_eps_and_u_match_oracle", "test_step_bce_kl_and_all_gradients_match_oracle",
        "test_thirty_adam_steps_through_the_beta_ramp_match_oracle", "test_mi_bounds_match_compute_batch_and_the_per_gate_loop"},
    "test_gpu_circuit_batched_kernels.py": {
        "test_fwd_and_bwd_batched_equal_the_single_kernels_and_the_oracle",
        "test_head_step_batched_equals_the_single_entry_and_a_float64_forward",
        "test_mi_bounds_batched_equal_the_single_kernel_and_compute_batch"},
    "test_gpu_circuit_ensemble.py": {
        "test_step_of_every_replica_matches_oracle", "test_thirty_adam_steps_through_per_replica_beta_ramps_match_oracle"},
    "test_gpu_dib_ensemble_kernels.py": {
        "test_reparam_forward_and_backward", "test_loss_and_history_sums", "test_posenc_rows_gathers_every_replica_and_feature"},
    "test_gpu_dib_ensemble.py": {
        "test_every_replicas_history_matches_the_oracle_fit_with_its_seeds_and_ramp", "test_gradients_of_both_replicas_match_the_oracle",
        "test_to_model_continues_the_replica_and_weight_access_round_trips", "test_an_mse_pair_with_two_outputs_matches_the_oracle"},
    "test_gpu_random_partition.py": {
        "test_kernel_matches_oracle_across_the_envelope", "test_duplicated_and_negated_columns_go_to_the_lower_index",
        "test_notebook_configurations_match_the_oracle", "test_logistic_generating_partition_known_answer"},
    "test_gpu_building_blocks.py": {
        "test_softmax_rows_forward_backward_vs_float64", "test_add_layernorm_forward_backward_vs_float64", "test_act_grad_mul_vs_numpy",
        "test_sgd_step_vs_numpy", "test_gemm_tile_shapes_the_default_rules_rarely_pick", "test_weight_gradient_flat_tile_vs_numpy", "test_attention_forward_with_projections_vs_float64", "test_attention_backward_with_projection_gradient_vs_float64"},
    "test_gpu_small_envelope.py": {"test_row_tile_envelope_step_matches_oracle", "test_paired_grid_matches_oracle"},
    "test_gpu_st_envelope.py": {"test_attention_envelope_matches_float64", "test_attention_with_projections_matches_float64",
                                "test_token_chain_envelope_matches_float64", "test_model_plan_branches_match_oracle"},
    "test_gpu_st_information.py": {
        "test_batched_sandwich_bounds_match_oracle", "test_probe_map_matches_oracle", "test_far_apart_gaussians_stay_finite",
        "test_notebook_batch_size_on_a_subset_of_probes", "test_information_bounds_match_the_oracle_on_the_model_encodings"},
    "test_gpu_mi_characterization.py": {
        "test_kernel_matches_oracle_across_the_envelope", "test_far_apart_gaussians_stay_finite",
        "test_bounds_from_parameters_equal_the_rows_loop_and_the_oracle", "test_known_answer_on_the_device"},
    "test_gpu_wgrad_stream.py": {"test_stream_kernel_slabs_are_the_tiled_kernels_bit_for_bit",
                                 "test_ineligible_shapes_stay_on_the_tiled_kernel",
                                 "test_bias_chains_of_the_128_column_tiled_kernel"},
    "test_gpu_wgrad_recompute.py": {"test_recompute_arm_has_the_stash_arms_bits", "test_two_bias_chains_of_the_large_launches"},
    "test_gpu_gemm_stream.py": {"test_forward_is_the_tiled_kernels_bit_for_bit", "test_dgrad_is_the_tiled_kernels_bit_for_bit",
                                "test_padded_leading_dimensions", "test_output_of_256_mb_is_stored_non_temporally_with_the_same_bits",
                                "test_ineligible_shapes_stay_on_the_tiled_kernel"},
    "test_gpu_input_grad.py": {"test_zoo_parity", "test_kernel_envelope", "test_grid_stride_rounds", "test_multi_tile_large_batch", "test_h1_not_stashed",
                               "test_addressing_and_guard_bands", "test_composition_upstream_module_gets_the_float64_gradient"},
    "test_gpu_feature_information.py": {
        "test_kernel_matches_oracle_across_the_envelope", "test_far_apart_gaussians_and_duplicated_rows",
        "test_information_per_feature_matches_oracle_on_every_dispatch_path",
        "test_validation_set_smaller_than_the_batch_draws_with_replacement"},
    "test_gpu_compression_matrices.py": {
        "test_kernel_matches_the_float64_oracle", "test_gather_equals_numpy",
        "test_model_matches_the_float64_chain_no_worse_than_the_loop"},
    "test_gpu_optimizers.py": {
        "test_every_rule_matches_the_float64_restatement", "test_envelope_of_sizes",
        "test_fit_with_rmsprop_matches_the_float64_oracle_fit", "test_fit_infonce_with_nadam_matches_the_float64_loop_oracle"},
    "test_gpu_grad_transforms.py": {
        "test_envelope_matches_the_float64_restatement", "test_real_layouts",
        "test_two_buffers_sharing_one_ss_array_take_the_norm_of_their_union", "test_learning_rate_on_the_device",
        "test_eight_steps_with_the_rules_match_the_composed_restatement",
        "test_fit_with_global_clipnorm_and_exponential_decay_matches_the_float64_oracle_fit",
        "test_fit_infonce_with_clipnorm_matches_the_float64_loop_oracle"},
    "test_gpu_losses.py": {
        "test_envelope_matches_the_float64_helper", "test_edges_stay_finite_and_gradients_vanish_where_the_contract_says",
        "test_one_training_step_matches_the_oracle_backward", "test_fit_under_huber_with_mae_matches_the_oracle_fit",
        "test_fit_on_one_hot_labels_with_smoothing_and_accuracy_matches_the_oracle_fit"},
    "test_gpu_tabular.py": {
        "test_envelope_matches_the_float64_oracle", "test_crafted_values", "test_fixture_through_the_device_backend",
        "test_table_end_to_end_against_the_oracle_fit"},
    "test_gpu_subset_information.py": {
        "test_device_matches_the_host_backend_across_the_envelope", "test_multi_bit_features",
        "test_every_fold_width_forced_through_its_tuning_key", "test_known_answers_are_exact",
        "test_paper_circuit_matches_the_notebook_and_ranks_its_printed_sequence", "test_random_circuit_of_14_gates"},
    "test_gpu_ctw_levels.py": {
        "test_grid_status_node_counts_and_rates", "test_grid_unrounded_code_length",
        "test_edges_short_windows_single_symbol_alphabet_and_sixteen_symbols",
        "test_75_logistic_windows_in_one_call_against_the_host_batch"},
}
# tests that demand the bits (or fp32 summation-order tolerance) of a path the tests above check against an oracle
EQUIVALENCE_TESTS = {
    "test_gpu_parity.py": {
        "test_companion_grids_equal_the_separate_launches", "test_fused_output_head_equals_the_unfused_sequence",
        "test_step_tail_equals_the_separate_launches", "test_small_batch_row_tile_kernels_equal_the_large_batch_path",
        "test_workspace_needs_only_dib_workspace_init", "test_inference_forward_skips_stashes_but_not_results"},
    "test_gpu_set_transformer.py": {
        "test_attention_backward_8_waves_equals_4_waves", "test_token_chain_kernels_equal_the_layer_by_layer_path",
        "test_deferred_grouped_weight_gradients_equal_the_per_block_launches",
        "test_graph_replay_of_the_train_step_is_bit_identical_to_eager",
        "test_evaluation_forward_skips_the_score_stash_and_backward_still_agrees",
        "test_data_parallel_shards_reproduce_the_full_batch_gradient", "test_large_token_count_uses_split_weight_gradients"},
    "test_gpu_dp_and_cache.py": {
        "test_fit_under_rccl_one_rank_equals_single_process", "test_three_bucket_backward_hooks_equal_the_plain_backward",
        "test_set_transformer_train_step_under_rccl_one_rank_equals_single_process"},
    "test_gpu_concurrency.py": {"test_two_threads_two_streams_equal_the_serial_run"},
    "test_gpu_wgrad_recompute.py": {"test_gates_keep_the_stash_path", "test_staged_backward_equals_the_single_call",
                                    "test_the_backward_follows_the_forwards_record", "test_enc_h_view_is_filled_on_demand"},
    "test_gpu_input_grad.py": {"test_bridge_returns_dx_and_leaves_the_parameter_gradients_alone"},
    "test_gpu_gemm_stream.py": {"test_relu_mask_values", "test_whole_step_has_the_tiled_arms_bits"},
    "test_gpu_st_information.py": {
        "test_batched_sandwich_equals_the_per_batch_rows_loop", "test_probe_map_equals_the_probe_bounds_loop",
        "test_information_maps_equal_information_map", "test_replay_is_bit_identical_and_bad_arguments_are_refused",
        "test_tracked_fit_trains_exactly_like_the_untracked_fit"},
    "test_gpu_mi_characterization.py": {
        "test_replay_split_calls_and_refusals", "test_bounds_from_parameters_reproduce_the_separation_zero_anchors",
        "test_characterize_on_a_small_sweep"},
    "test_gpu_feature_information.py": {
        "test_kernel_equals_the_sandwich_rows_loop", "test_replay_and_splits_are_bit_identical",
        "test_chunks_of_batches_do_not_change_the_bits",
        "test_all_features_equal_the_per_feature_loop_and_a_shape_beyond_the_envelope_takes_it",
        "test_callback_in_one_launch_fills_bounds_like_information_per_feature",
        "test_tracked_fit_trains_exactly_like_the_untracked_fit"},
    "test_gpu_compression_matrices.py": {
        "test_matrices_equal_their_transposes_bit_for_bit", "test_one_output_alone_gives_the_same_bits",
        "test_replay_placement_and_feature_splits_are_bit_identical",
        "test_a_shape_beyond_the_envelope_takes_the_loop_and_equals_it",
        "test_callback_one_launch_and_loop_agree_and_neither_changes_the_training"},
    "test_gpu_optimizers.py": {
        "test_buckets_then_one_advance_equal_the_whole_buffer_step",
        "test_captured_steps_replay_bit_identically_and_advance_t_and_P"},
    "test_gpu_grad_transforms.py": {
        "test_buckets_in_any_order_give_the_bits_of_the_whole_buffer", "test_a_captured_step_replays_with_an_advancing_learning_rate",
        "test_unchanged_paths_keep_their_launches_and_their_bits",
        "test_fit_with_global_clipnorm_under_rccl_one_rank_equals_single_process"},
    "test_gpu_losses.py": {
        "test_bits_do_not_depend_on_the_call_or_the_block", "test_fit_under_graph_replay_has_the_eager_bits_for_a_new_kind"},
    "test_gpu_tabular.py": {
        "test_placement_does_not_change_the_bits", "test_graph_replay_has_the_eager_bits",
        "test_fit_on_a_device_tensor_equals_fit_on_numpy_bit_for_bit"},
    "test_gpu_subset_information.py": {"test_chunks_and_placement_do_not_change_the_bits", "test_graph_replay_has_the_eager_bits"},
    "test_gpu_measurement_ensemble.py": {
        "test_a_replica_does_not_see_the_others", "test_fit_retires_replicas_at_their_own_thresholds",
        "test_one_replica_as_a_model_and_its_symbols"},
    "test_gpu_circuit_batched_kernels.py": {"test_65_replicas_in_two_launches_equal_65_single_calls"},
    "test_gpu_circuit_ensemble.py": {
        "test_one_replica_equals_the_single_model_bit_for_bit", "test_a_replica_does_not_see_the_others",
        "test_fit_is_reproducible_and_evaluates_like_the_single_model", "test_to_model_continues_a_replica_with_the_same_bits"},
    "test_gpu_dib_ensemble_kernels.py": {"test_forward_reproduces_a_single_engines_u_bit_for_bit"},
    "test_gpu_dib_ensemble.py": {"test_a_replica_does_not_see_the_others"},
    "test_gpu_ctw_levels.py": {
        "test_chunks_do_not_change_the_bits_and_an_overflowing_window_goes_to_the_host",
        "test_entropy_rate_fit_on_the_device_backend", "test_random_partition_characterize_keeps_the_symbols_on_the_device"},
}


def _kind(nodeid):
    """'*' oracle-comparing, '=' equivalence with an oracle-checked path, ' ' other"""
    parts = nodeid.split("::")
    f, fn = os.path.basename(parts[0]), parts[-1].split("[")[0]
    if fn in ORACLE_TESTS.get(f, ()):
        return "*"
    if fn in EQUIVALENCE_TESTS.get(f, ()):
        return "="
    return " "


def library_kernels(lib=LIB):
    """Mangled names of the kernels in the library's gfx950 code object (the .kd kernel-descriptor symbols)."""
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", lib, os.path.join(d, "x")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fb}", f"--output={co}"], check=True)
        out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split()
        if parts and parts[-1].endswith(".kd"):
            names.add(parts[-1][:-3])
    return sorted(names)


def demangle(names):
    import shutil
    cxxfilt = next((c for c in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if c and os.path.exists(c)), None)
    if cxxfilt is None:
        return {n: n for n in names}
    out = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def _read_ranges(trace_dir, tests_tsv):
    """[(start, end, nodeid)] in the profiler's clock: ROCTx ranges if the marker trace has them, else the host-clock log."""
    ranges = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*marker_api_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = next((v for v in row.values() if isinstance(v, str) and v.startswith("dibtest::")), None)
                if name:
                    ranges.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name[len("dibtest::"):]))
    if ranges:
        return sorted(ranges), "ROCTx ranges (rocprofv3 --marker-trace)"
    return None, None


def _ranges_from_clock_log(tests_tsv, kstart_min, kstart_max):
    rows = [l.rstrip("\n").split("\t") for l in open(tests_tsv)]
    best = None
    for c, label in enumerate(("CLOCK_MONOTONIC", "CLOCK_BOOTTIME", "CLOCK_REALTIME")):
        r = sorted((int(x[1 + c]), int(x[4 + c]), x[0]) for x in rows)
        if r and r[0][0] <= kstart_min and kstart_max <= r[-1][1]:
            best = (r, f"host clock log ({label})")
            break
    if best is None:
        raise SystemExit("no clock of the host log brackets the kernel timestamps and the marker trace is empty")
    return best


def build(trace_dir, tests_tsv, out_path):
    disp = []   # (start, name)
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if name.endswith(".kd"):
                    name = name[:-3]
                disp.append((int(row["Start_Timestamp"]), name))
    disp.sort()
    ranges, how = _read_ranges(trace_dir, tests_tsv)
    if ranges is None:
        ranges, how = _ranges_from_clock_log(tests_tsv, disp[0][0], disp[-1][0])
    starts = [r[0] for r in ranges]
    by_kernel = {}
    unassigned = 0
    for t, name in disp:
        i = bisect.bisect_right(starts, t) - 1
        while i >= 0 and ranges[i][1] < t:   # ranges of one pytest process do not nest; step back over finished ones
            i -= 1
            if i < 0 or ranges[i][0] + 10**12 < t:
                i = -1
                break
        if i < 0:
            unassigned += 1
            continue
        d = by_kernel.setdefault(name, {})
        d[ranges[i][2]] = d.get(ranges[i][2], 0) + 1
    lib_kernels = library_kernels()
    dm = demangle(lib_kernels)
    lines = ["# kernel coverage of `python -m pytest tests -m gpu` under rocprofv3 --kernel-trace --marker-trace -M",
             f"# test ranges from: {how}; {len(disp)} dispatches, {unassigned} outside every test range (session set-up)",
             f"# {len(lib_kernels)} kernel symbols in libdib_hip.so (gfx950 code object); '*' = the test compares with the float64 / NumPy oracle,",
             "# '=' = the test demands equality (bits or fp32 summation-order tolerance) with a path that '*' tests check",
             "# format: KERNEL <mangled>  |  <demangled>  |  launches  |  tests  |  '*' tests  |  '=' tests ; then one line per test (at most 12, '*' first)"]
    missing = []
    for k in lib_kernels:
        tests = by_kernel.get(k, {})
        oracle = [t for t in tests if _kind(t) == "*"]
        equiv = [t for t in tests if _kind(t) == "="]
        lines.append(f"KERNEL {k}  |  {dm[k]}  |  {sum(tests.values())}  |  {len(tests)}  |  {len(oracle)}  |  {len(equiv)}")
        if not tests:
            missing.append(k)
        order = sorted(tests, key=lambda t: ("*= ".index(_kind(t)), t))
        for t in order[:12]:
            lines.append(f"    {_kind(t)} {t}  ({tests[t]})")
        if len(order) > 12:
            lines.append(f"      ... and {len(order) - 12} more tests")
    other = sorted(k for k in by_kernel if k not in set(lib_kernels))
    lines.append(f"# kernels launched by the suite that are not the library's (torch / RCCL): {len(other)}")
    lines.append(f"# library kernels no test launched: {len(missing)}")
    for k in missing:
        lines.append(f"MISSING {k}  |  {dm[k]}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{out_path}: {len(lib_kernels)} kernels, {len(missing)} not launched, {unassigned} dispatches unassigned")


def merge(out_path, *part_paths):
    """One record from the records of parts of the suite that share no test (each part `build`s against the same library):
    launches and test counts add up, the test lines are re-sorted together ('*' first) and cut to 12 again - every part lists
    its own first 12 in that order, so the merged first 12 are among them."""
    import re
    kernels, order, dispatches, unassigned, other, n_parts = {}, [], 0, 0, 0, 0
    for path in part_paths:
        cur = None
        merged = [int(m.group(1)) for m in (re.search(r", (\d+) parts of the suite merged;", l) for l in open(path)) if m]
        n_parts += merged[0] if merged else 1     # (a record that is itself a merge counts with all its parts)
        for line in open(path):
            line = line.rstrip("\n")
            m = re.match(r"# test ranges from: .*; (\d+) dispatches, (\d+) outside", line)
            if m:
                dispatches, unassigned = dispatches + int(m.group(1)), unassigned + int(m.group(2))
            m = re.match(r"# kernels launched by the suite that are not the library's \(torch / RCCL\): (\d+)", line)
            if m:
                other = max(other, int(m.group(1)))
            if line.startswith("KERNEL "):
                parts = [p.strip() for p in line[len("KERNEL "):].split("  |  ")]
                if parts[0] not in kernels:
                    kernels[parts[0]] = dict(dm=parts[1], n=[0, 0, 0, 0], tests={})
                    order.append(parts[0])
                cur = kernels[parts[0]]
                for i in range(4):
                    cur["n"][i] += int(parts[2 + i])
            elif cur is not None and line.startswith("    ") and line.rstrip().endswith(")") and "... and" not in line:
                m = re.match(r"    (.) (.*)  \((\d+)\)$", line)
                cur["tests"][m.group(2)] = (m.group(1), int(m.group(3)))
            elif not line.startswith("    "):
                cur = None
    lines = ["# kernel coverage of `python -m pytest tests -m gpu` under rocprofv3 --kernel-trace --marker-trace -M",
             f"# test ranges from: ROCTx ranges (rocprofv3 --marker-trace), {n_parts} parts of the suite merged; {dispatches} dispatches, "
             f"{unassigned} outside every test range (session set-up)",
             f"# {len(order)} kernel symbols in libdib_hip.so (gfx950 code object); '*' = the test compares with the float64 / NumPy oracle,",
             "# '=' = the test demands equality (bits or fp32 summation-order tolerance) with a path that '*' tests check",
             "# format: KERNEL <mangled>  |  <demangled>  |  launches  |  tests  |  '*' tests  |  '=' tests ; then one line per test (at most 12, '*' first)"]
    missing = []
    for k in sorted(order):
        e = kernels[k]
        lines.append(f"KERNEL {k}  |  {e['dm']}  |  {e['n'][0]}  |  {e['n'][1]}  |  {e['n'][2]}  |  {e['n'][3]}")
        if e["n"][1] == 0:
            missing.append(k)
        names = sorted(e["tests"], key=lambda t: ("*= ".index(e["tests"][t][0]), t))
        for t in names[:12]:
            lines.append(f"    {e['tests'][t][0]} {t}  ({e['tests'][t][1]})")
        if e["n"][1] > 12:
            lines.append(f"      ... and {e['n'][1] - 12} more tests")
    lines.append(f"# kernels launched by the suite that are not the library's (torch / RCCL): {other}")
    lines.append(f"# library kernels no test launched: {len(missing)}")
    for k in missing:
        lines.append(f"MISSING {k}  |  {kernels[k]['dm']}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{out_path}: {len(order)} kernels, {len(missing)} not launched")


def read_record(path):
    """{mangled kernel: (launches, number of tests, number of oracle-comparing tests, number of equivalence tests)}"""
    rec = {}
    for line in open(path):
        if line.startswith("KERNEL "):
            parts = [p.strip() for p in line[len("KERNEL "):].split("  |  ")]
            rec[parts[0]] = (int(parts[2]), int(parts[3]), int(parts[4]), int(parts[5]) if len(parts) > 5 else 0)
    return rec


def check(path):
    rec = read_record(path)
    bad = [k for k in library_kernels() if rec.get(k, (0, 0, 0, 0))[1] == 0]
    for k in bad:
        print("not covered:", k)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build(*sys.argv[2:5])
    elif sys.argv[1] == "merge":
        merge(sys.argv[2], *sys.argv[3:])
    elif sys.argv[1] == "check":
        sys.exit(check(sys.argv[2]))
    elif sys.argv[1] == "list":
        for k, v in demangle(library_kernels()).items():
            print(k, " | ", v)
