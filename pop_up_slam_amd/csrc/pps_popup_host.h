// pps_popup_host.h -- what other host files of the library may read of a pps_popup (the struct itself stays private to pps_popup.hip).
#pragma once
#include "../../include/pps.h"

namespace pps {

// the last pps_popup_run / _run_async of a context: its device buffers, valid until the next run of the same context
struct PopupRunView {
  int device, width, height, step;
  const pps_point* cloud;      // width * height, every pixel written (valid bit = bit 24 of rgba)
  const int* plane_id;         // width * height, -1 = none
  const float* T_wc;           // the 16 floats the run was given (row-major, sensor -> world)
};
// PPS_ESTATE (answered on the host, before anything is waited for): no run yet, or the run had the plane-id output switched off.
// A run in flight is waited for, like every reader of a run does.  The message goes to pps_popup_last_error(p).
int popup_last_run(pps_popup* p, PopupRunView* v);

}  // namespace pps
