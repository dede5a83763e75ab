// gpsat_select_types.h -- the plain structs that the selection's host planning (gpsat_select_plan.h) shares with its kernels
// (gpsat_kernels.h, gpsat_select.hip).  No HIP header: gpsat_select_plan.h compiles with a plain host compiler.
#ifndef GPSAT_SELECT_TYPES_H
#define GPSAT_SELECT_TYPES_H

#define GPSAT_SEL_MAXCRIT 4

namespace gpsat {

// The criteria of a selection, checked and normalised (select_check_spec).  The first fields of SelectArgs.
struct SelectCriteria {
    int n_crit;
    int kind[GPSAT_SEL_MAXCRIT];      // 0: 1-D compare, 1: Euclidean ball, 2: per-expert interval on cols[k][0], bounds cols[k][1]
    int comp[GPSAT_SEL_MAXCRIT];      // 0 >=, 1 >, 2 ==, 3 <, 4 <=
    int ncols[GPSAT_SEL_MAXCRIT];
    int cols[GPSAT_SEL_MAXCRIT][3];
    double val[GPSAT_SEL_MAXCRIT];
};

// Spatial binning of the point table (gpsat_select.hip): rows sorted by the cell of up to 3 columns, so that the boxes of
// consecutive rows are tight whatever order the table came in.
struct BinSpec {
    int ndim;                         // binned columns (1..3)
    int col[3];
    double origin[3], inv_cell[3];
    int ncell[3];
};

}  // namespace gpsat
#endif
