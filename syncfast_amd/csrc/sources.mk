# The library's translation units by base name, for every Makefile that builds
# it (this directory's, and examples/Makefile's sanitizer build).
# GPU: compiled by hipcc, each into a code object of its own.
SF_GPU := sf_capi sf_stream sf_chain sf_sort sf_table sf_match sf_wire sf_litmus sf_cdc sf_cdc_files sf_recv sf_recv_data sf_recv_files sf_copy sf_send sf_want sf_send_files sf_names sf_send_entries sf_recv_entries sf_serve_files sf_plan_copies
# Host: the HIP runtime API only, no kernels.
SF_HOST := sf_batch sf_host sf_host_out sf_pagelock sf_files sf_fds sf_fds_zpaq sf_stage sf_multi sf_pool sf_cut sf_knobs sf_alloc
# Host, and no HIP header either.
SF_HOST_PLAIN := sf_zpaq host_sha1
