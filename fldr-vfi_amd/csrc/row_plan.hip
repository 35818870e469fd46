// fldr_synth_row_plan (include/fldr_hip.h): host code only, the rules are in row_plan.h.
#include "row_plan.h"

extern "C" int fldr_synth_row_plan(int H, int Hc, fldr_synth_rows* plan) { return fldr_plan_rows(H, Hc, plan); }
