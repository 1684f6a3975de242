// variants/diag_uniform_visit.inc -- SHRAY_DIAG_UNIFORM: included inside inner_stage's turn (wave_traversal.h) by the diagnostic build only.
// VERDICT round 5, item 2: of the wave-visits whose walking lanes are all at ONE record (the ones the scalar cache serves), how many
// end with the same decision in every lane -- what a packet-level (scalar interval) decision could settle without the per-lane test.
{
    const unsigned long long walkers = wave_ballot(true);
    const uint32_t at = node_address(t, t.node);
    const bool uniform = wave_ballot(at != (uint32_t)__builtin_amdgcn_readfirstlane((int)at)) == 0ull;
    float d0, d1;
    uint32_t da = __float_as_uint(lo.w), db = __float_as_uint(hi.w);
    const bool enters = visit_decision(t, lo, hi, d0, d1, da, db);
    const unsigned long long entering = wave_ballot(enters);
    diag_tally_ref[0] += 1;
#ifndef SHRAY_DIAG_UNIFORM_ORIGIN
    diag_tally_ref[7] += (unsigned long long)__popcll(walkers);
#endif
    if (uniform) {
        diag_tally_ref[1] += 1;
        diag_tally_ref[entering == walkers ? 2 : (entering == 0ull ? 3 : 4)] += 1;
    }
#ifdef SHRAY_DIAG_UNIFORM_ORIGIN
    // Round 8 (R8.1): where the "no lane enters" uniform visits come from.  diag_chain counts the words that uniform
    // every-lane-enters-a-branch turns of THIS stage call have pushed, one after the other, and that are still every walking lane's
    // topmost stack entries; any turn that is neither such a push nor a uniform no-lane-enters pop out of the chain ends it.
    // tally 5: pops that directly follow such a push -- low word: push and pop within one group of SHRAY_NODE_TURNS turns (what a
    // one-deep scalar mirror serves), high word: the pop is a group's first turn (the exit tests lie between the two);
    // tally 6: pops at one remove or more (a further pop out of the same chain); tally 7: uniform every-lane-enters turns at a
    // LEAF's record.  (Turns the scheduled stage hands to the compiler's visit are not told apart here: an upper bound.)
    if (uniform && entering == walkers && !(db & kLeafFlag)) {
        diag_chain++;
        diag_popped = false;
    } else if (uniform && entering == 0ull && diag_chain > 0) {
        if (diag_popped)
            diag_tally_ref[6] += 1;
        else
            diag_tally_ref[5] += turn != 0 ? 1ull : 1ull << 32;
        diag_chain--;
        diag_popped = true;
    } else {
        diag_chain = 0;
        if (uniform && entering == walkers)
            diag_tally_ref[7] += 1;
    }
#else
    if (!uniform) {
        // how many distinct records the walking lanes are at (what a vector-memory instruction of this visit reads): 2, 3-4, more
        // -- the classes bench.py prices the kernel's vector-memory instructions with (profiles/make_vmem_mix.py)
        int distinct = 0;
        unsigned long long left = walkers;
        while (left != 0ull && distinct < 5) {
            const uint32_t one = (uint32_t)__builtin_amdgcn_readlane((int)at, __builtin_ctzll(left));
            left &= ~wave_ballot(at == one);
            distinct++;
        }
        if (distinct == 2)
            diag_tally_ref[5] += 1;
        else if (distinct <= 4)
            diag_tally_ref[6] += 1;
    }
#endif
}
