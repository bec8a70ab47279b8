// reservoir.hip, for readout.hip: what a launch over a reservoir's segment records needs of the handle.
#pragma once

struct lsm_reservoir;       // the reservoir handle (reservoir.hip)

struct ReservoirRecordFacts {
    int n_out;              // output neurons: records per segment
    int burst_isi_max;      // SPEC.md §4's burst limit, which merging two records needs
    int device;             // the device the handle lives on
};

ReservoirRecordFacts reservoir_record_facts(const lsm_reservoir *h);
