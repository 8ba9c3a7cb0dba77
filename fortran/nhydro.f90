!> Drop-in replacement of the reference's model-facing module (src/nhydro.f90): same module name, same five
!> procedures with the same argument lists, bodies forwarding through ISO_C_BINDING to libmgx.so (include/mgx.h),
!> whose operators are HIP kernels on the MI355X.  An ocean model (or the reference's own mg_testseamount driver)
!> that does `use nhydro` links against this object + libmgx.so instead of the reference's solver modules.
!>
!> Like the reference's module, it re-exports what it uses (fortran/mg_solvers.f90): the solver-level procedures solve_p, Fcycle,
!> Vcycle, Vcycle2, testgalerkin, relax, compute_residual, fine2coarse, coarse2fine, fill_halo, tic / toc / print_tictoc, and the
!> module variables myrank, nlevs, netcdf_output, bmask ... -- what the reference's drivers take through `use nhydro`
!> (mg_testseamount.f90:37,201,220-221; old_tests/mg_testrelax.f90).  grid(lev)%p becomes grid_get(lev,'p',array).
!>
!> The namelist ./nh_namelist is read by the library (same members, mg_namelist.f90:37-50); rank 0 prints the same parameter
!> block / level table / "ite = " lines.  Multi-rank runs need the three communication hooks of mgx_set_comm (INTEGRATION.md;
!> fortran/mgx_mpi_hooks.cpp serves them with MPI); set `myrank` before nhydro_init.
module nhydro
  use iso_c_binding
  use mgx_c
  use mg_tictoc
  use mg_mpi
  use mg_namelist
  use mg_grids
  use mg_mpi_exchange
  use mg_relax
  use mg_intergrids
  use mg_solvers
  implicit none

contains

  !--------------------------------------------------------------  (nhydro.f90:18-33)
  subroutine nhydro_init(nx, ny, nz, npxg, npyg)
    integer(kind=ip), intent(in) :: nx, ny, nz
    integer(kind=ip), intent(in) :: npxg, npyg
    call mgx_check(mgx_init(nx, ny, nz, npxg, npyg, myrank, c_null_ptr), 'nhydro_init')
    call mgx_namelist_readback()       ! netcdf_output, bmask, ns_pre ... as `use mg_namelist` gives the reference's drivers
    nlevs = mgx_nlevs()                ! mg_grids.f90:117
  end subroutine nhydro_init

  !--------------------------------------------------------------  (nhydro.f90:36-50)
  subroutine nhydro_matrices(dx, dy, zeta, h, rmask, hc, theta_b, theta_s)
    real(kind=rp), dimension(:,:)         , intent(in) :: dx, dy, zeta, h
    real(kind=rp), dimension(:,:), pointer, intent(in) :: rmask
    real(kind=rp)                         , intent(in) :: hc, theta_b, theta_s
    real(kind=rp), dimension(:,:), allocatable :: a, b, c, d   ! contiguous copies of the assumed-shape arguments
    real(kind=rp), dimension(:,:), allocatable, target :: m
    allocate(a, source=dx); allocate(b, source=dy); allocate(c, source=zeta); allocate(d, source=h)
    if (associated(rmask)) then   ! only read by the library when bmask=.true.
       allocate(m, source=rmask)
       call mgx_check(mgx_matrices(a, b, c, d, c_loc(m), hc, theta_b, theta_s), 'nhydro_matrices')
    else
       call mgx_check(mgx_matrices(a, b, c, d, c_null_ptr, hc, theta_b, theta_s), 'nhydro_matrices')
    endif
  end subroutine nhydro_matrices

  !--------------------------------------------------------------  (nhydro.f90:53-102)
  subroutine nhydro_solve(nx, ny, nz, rmaska, ua, va, wa)
    integer(kind=ip), intent(in) :: nx, ny, nz
    real(kind=rp), dimension(0:nx+1,0:ny+1)     , target, intent(inout) :: rmaska
    real(kind=rp), dimension(1:nx+1,0:ny+1,1:nz), target, intent(inout) :: ua
    real(kind=rp), dimension(0:nx+1,1:ny+1,1:nz), target, intent(inout) :: va
    real(kind=rp), dimension(0:nx+1,0:ny+1,0:nz), target, intent(inout) :: wa
    ! rmaska: the memory the caller allocated as rmask(0:ny+1,0:nx+1) and filled as rmask(j,i) (mg_testseamount.f90:97,185).  The
    ! library reads it in THAT layout (element (j,i) at j+(ny+2)*i).  The reference, after `rmask => rmaska` with the bounds declared
    ! above, reads rmask(j,i) at j+(nx+2)*i (nhydro.f90:72, mg_compute_rhs.f90:61,110): the same element for square blocks or an
    ! all-ones mask -- the cases it is run on -- and a different one otherwise.  Deliberate: the drivers' layout is the intent.
    call mgx_check(mgx_solve(ua, va, wa, c_loc(rmaska)), 'nhydro_solve')
  end subroutine nhydro_solve

  !--------------------------------------------------------------  (nhydro.f90:105-134)
  subroutine nhydro_check_nondivergence(nx, ny, nz, rmaska, ua, va, wa)
    integer(kind=ip), intent(in) :: nx, ny, nz
    real(kind=rp), dimension(0:nx+1,0:ny+1)     , target, intent(inout) :: rmaska
    real(kind=rp), dimension(1:nx+1,0:ny+1,1:nz), target, intent(inout) :: ua
    real(kind=rp), dimension(0:nx+1,1:ny+1,1:nz), target, intent(inout) :: va
    real(kind=rp), dimension(0:nx+1,0:ny+1,0:nz), target, intent(inout) :: wa
    call mgx_check(mgx_check_nondivergence(ua, va, wa, c_loc(rmaska)), 'nhydro_check_nondivergence')
  end subroutine nhydro_check_nondivergence

  !--------------------------------------------------------------  (no counterpart in the reference, whose state is real(kind=rp))
  ! The same two calls for a model that keeps u, v, w in single precision: each element comes back as real(x, 4) of the x that
  ! nhydro_solve leaves when it is given real(ua, 8), real(va, 8), real(wa, 8) -- b, p and the iteration count are those of that
  ! call, bit for bit (include/mgx.h: the float state).  The mask stays real(kind=rp).
  subroutine nhydro_solve_r4(nx, ny, nz, rmaska, ua, va, wa)
    integer(kind=ip), intent(in) :: nx, ny, nz
    real(kind=rp), dimension(0:nx+1,0:ny+1)     , target, intent(inout) :: rmaska
    real(c_float), dimension(1:nx+1,0:ny+1,1:nz), target, intent(inout) :: ua
    real(c_float), dimension(0:nx+1,1:ny+1,1:nz), target, intent(inout) :: va
    real(c_float), dimension(0:nx+1,0:ny+1,0:nz), target, intent(inout) :: wa
    call mgx_check(mgx_solve_f32(ua, va, wa, c_loc(rmaska)), 'nhydro_solve_r4')
  end subroutine nhydro_solve_r4

  subroutine nhydro_check_nondivergence_r4(nx, ny, nz, rmaska, ua, va, wa)
    integer(kind=ip), intent(in) :: nx, ny, nz
    real(kind=rp), dimension(0:nx+1,0:ny+1)     , target, intent(inout) :: rmaska
    real(c_float), dimension(1:nx+1,0:ny+1,1:nz), target, intent(inout) :: ua
    real(c_float), dimension(0:nx+1,1:ny+1,1:nz), target, intent(inout) :: va
    real(c_float), dimension(0:nx+1,0:ny+1,0:nz), target, intent(inout) :: wa
    call mgx_check(mgx_check_nondivergence_f32(ua, va, wa, c_loc(rmaska)), 'nhydro_check_nondivergence_r4')
  end subroutine nhydro_check_nondivergence_r4

  !--------------------------------------------------------------  (no counterpart in the reference, whose model lives on the host)
  ! The set-up half of a time step for a model that keeps its state on the GPU: every argument is the DEVICE address of an array in the
  ! layout of the host call of the same name (c_null_ptr for an absent rmask).  nhydro_update_zeta_device is the per-step call: a new
  ! zeta under the dx, dy, h, rmask, hc, theta_b, theta_s of the last nhydro_matrices / nhydro_matrices_device (include/mgx.h).
  subroutine nhydro_matrices_device(dx, dy, zeta, h, rmask, hc, theta_b, theta_s)
    type(c_ptr), value, intent(in) :: dx, dy, zeta, h, rmask
    real(kind=rp), intent(in) :: hc, theta_b, theta_s
    call mgx_check(mgx_matrices_device(dx, dy, zeta, h, rmask, hc, theta_b, theta_s), 'nhydro_matrices_device')
  end subroutine nhydro_matrices_device

  subroutine nhydro_update_zeta_device(zeta)
    type(c_ptr), value, intent(in) :: zeta
    call mgx_check(mgx_update_zeta_device(zeta), 'nhydro_update_zeta_device')
  end subroutine nhydro_update_zeta_device

  subroutine nhydro_check_nondivergence_device(rmaska, ua, va, wa)
    type(c_ptr), value, intent(in) :: rmaska, ua, va, wa
    call mgx_check(mgx_check_nondivergence_device(ua, va, wa, rmaska), 'nhydro_check_nondivergence_device')
  end subroutine nhydro_check_nondivergence_device

  !--------------------------------------------------------------  (no counterpart in the reference, which evaluates its own stretching)
  ! nhydro_matrices for a model that owns its vertical grid: instead of zeta, h and the sigma parameters, the depths of level 1 in the
  ! layout grid_get(1,'zr',.) / grid_get(1,'zw',.) return, zr(nz,-1:ny+2,-1:nx+2) and zw(nz+1,-1:ny+2,-1:nx+2).  Only the columns
  ! j = 1..ny, i = 1..nx are read; the coarser levels' depths are averages of these (include/mgx.h: mgx_matrices_depths).
  subroutine nhydro_matrices_depths(dx, dy, zr, zw, rmask)
    real(kind=rp), dimension(:,:)         , intent(in) :: dx, dy
    real(kind=rp), dimension(:,:,:)       , intent(in) :: zr, zw
    real(kind=rp), dimension(:,:), pointer, intent(in) :: rmask
    real(kind=rp), dimension(:,:), allocatable :: a, b           ! contiguous copies of the assumed-shape arguments
    real(kind=rp), dimension(:,:,:), allocatable :: c, d
    real(kind=rp), dimension(:,:), allocatable, target :: m
    allocate(a, source=dx); allocate(b, source=dy); allocate(c, source=zr); allocate(d, source=zw)
    if (associated(rmask)) then   ! only read by the library when bmask=.true.
       allocate(m, source=rmask)
       call mgx_check(mgx_matrices_depths(a, b, c, d, c_loc(m)), 'nhydro_matrices_depths')
    else
       call mgx_check(mgx_matrices_depths(a, b, c, d, c_null_ptr), 'nhydro_matrices_depths')
    endif
  end subroutine nhydro_matrices_depths

  ! ... and for a model that keeps them on the GPU: DEVICE addresses; strides = c_null_ptr for the layout above, else the address of the four
  ! integer(c_long_long) zr_sj, zr_sk, zw_sj, zw_sk of the model's own i-fastest padded arrays, zr and zw then naming z_r(1,1,1) and
  ! z_w(1,1,0).  nhydro_update_depths_device is the per-step call: new depths under the dx, dy, rmask of the last set-up.
  subroutine nhydro_matrices_depths_device(dx, dy, zr, zw, strides, rmask)
    type(c_ptr), value, intent(in) :: dx, dy, zr, zw, strides, rmask
    call mgx_check(mgx_matrices_depths_device(dx, dy, zr, zw, strides, rmask), 'nhydro_matrices_depths_device')
  end subroutine nhydro_matrices_depths_device

  subroutine nhydro_update_depths_device(zr, zw, strides)
    type(c_ptr), value, intent(in) :: zr, zw, strides
    call mgx_check(mgx_update_depths_device(zr, zw, strides), 'nhydro_update_depths_device')
  end subroutine nhydro_update_depths_device

  !--------------------------------------------------------------  (nhydro.f90:137-141)
  subroutine nhydro_clean()
    call mgx_clean()
  end subroutine nhydro_clean

end module nhydro
