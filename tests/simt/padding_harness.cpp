// tilesort_harness.cpp plus the two ranking options of csrc/gsr_internal.h (ranking_generic, ranking_pad_last) and the hook that names the
// instantiations the launchers chose -- for tests/test_simt_ranking_padding_cpu.py.  TEST INFRASTRUCTURE: built into tests/_build/, never part of libgsr_hip.so.
#include "tilesort_harness.cpp"

extern "C" {

void simt_set_ranking(int generic, int pad_last) {
    gsr_set_ranking_generic(generic);
    gsr_set_ranking_pad_last(pad_last);
}

// hb << 4 | lb of the most recent emit_scatter / bucket_scatter launches (0: the run-time-width kernels)
int simt_last_ranking_widths(void) { return g_ranking_last_hb << 4 | g_ranking_last_lb; }

}  // extern "C"
