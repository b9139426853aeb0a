// emu_lalign.cpp -- TEST INFRASTRUCTURE (tests/test_lalign_cpu.py): the left-alignment routine of the device sources
// (lamsa_amd/csrc/hp_lalign.h) on explicit inputs under the CPU lane emulation.  The whole per-read path with result tags set is
// emu_align_batch_tags of emu_eqx.cpp, which is included as it is and brings emu_api.cpp (the emulation's globals, LDS guards, sort
// widths) with it.
#include "emu_eqx.cpp"

// One record: cig[0 .. cn) (M form) is left-aligned in place against the read on the record's strand (rl base codes) and the forward
// reference from the record's offset (tl base codes).  The routine sees exact-size copies of the two sequences, so a read outside either
// is a read outside an allocation.  Returns the number of gaps the routine says it moved.
extern "C" int emu_lalign_record(int32_t *cig, int cn, const uint8_t *read, int rl, const uint8_t *ref, int tl)
{
    std::vector<uint8_t> R(read, read + rl), T(ref, ref + tl);
    return lalign_cigar((cig_t *)cig, cn, R.data(), rl, T.data(), tl);
}
