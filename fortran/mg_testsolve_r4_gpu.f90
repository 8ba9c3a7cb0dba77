!> The float state through the Fortran boundary (nhydro_solve_r4, fortran/nhydro.f90): the seamount at 32x32x8, four colours to 1e-8,
!> u = v = 0, w = -1 plus a perturbation that single precision holds exactly, solved once with the state in real(8) (nhydro_solve) and
!> once in real(4) (nhydro_solve_r4).  The contract of include/mgx.h says the real(4) result is the real(8) one rounded once, so the
!> program prints how many elements of real(u8, 4) and u4 differ in their bits (likewise v, w: each count must be 0) and the two
!> iteration counts (equal).  The counts are read from the history file fort.100, which the library writes per solve.
!> Parameters: ./nh_namelist when there is one (the tests write it), else the program writes the one named above.
program mg_testsolve_r4_gpu
  use iso_c_binding
  use nhydro
  implicit none
  integer(kind=4), parameter :: nx = 32, ny = 32, nz = 8
  integer(kind=4) :: i, j, k, nite8, nite4
  real(kind=8) :: Lx, Ly, Htot, hc, theta_b, theta_s, x, y, x0, y0
  real(kind=8), dimension(:,:), pointer :: dx, dy, zeta, h, rmask
  real(kind=8), dimension(:,:,:), allocatable :: u8, v8, w8
  real(kind=4), dimension(:,:,:), allocatable :: u4, v4, w4
  logical :: there

  inquire(file='nh_namelist', exist=there)
  if (.not. there) then
     open(unit=21, file='nh_namelist', status='new', action='write')
     write(21,'(A)') '&nhparam', " relax_method = 'FC',", ' solver_prec = 1.d-8,', '/'
     close(21)
  endif
  call forget_history()

  call nhydro_init(nx, ny, nz, 1, 1)
  Lx = 1.e4_8; Ly = 1.e4_8; Htot = 4.e3_8
  hc = 4.e3_8; theta_b = 0._8; theta_s = 0._8
  allocate(dx(0:ny+1,0:nx+1), dy(0:ny+1,0:nx+1), zeta(0:ny+1,0:nx+1), h(0:ny+1,0:nx+1), rmask(0:ny+1,0:nx+1))
  dx(:,:) = Lx/real(nx,kind=8); dy(:,:) = Ly/real(ny,kind=8); zeta(:,:) = 0._8; rmask(:,:) = 1._8
  x0 = Lx*0.5_8; y0 = Ly*0.5_8
  do i = 0, nx+1                              ! mg_setup_tests.f90:139-148
     do j = 0, ny+1
        x = (real(i,kind=8)-0.5_8)*dx(j,i)
        y = (real(j,kind=8)-0.5_8)*dy(j,i)
        h(j,i) = Htot*(1._8 - 0.5_8*exp(-(x-x0)**2._8/(Lx/5._8)**2._8 - (y-y0)**2._8/(Ly/5._8)**2._8))
     enddo
  enddo
  if (bmask) call fill_halo_2D_bmask(1, rmask)
  call nhydro_matrices(dx, dy, zeta, h, rmask, hc, theta_b, theta_s)

  ! the state: multiples of 1/64 of a few units, exact in real(4)
  allocate(u4(1:nx+1,0:ny+1,1:nz), v4(0:nx+1,1:ny+1,1:nz), w4(0:nx+1,0:ny+1,0:nz))
  do k = 1, nz
     do j = 0, ny+1
        do i = 1, nx+1
           u4(i,j,k) = real(mod(7*i + 3*j + 5*k, 11) - 5, 4) / 64._4
        enddo
     enddo
     do j = 1, ny+1
        do i = 0, nx+1
           v4(i,j,k) = real(mod(5*i + 7*j + 3*k, 13) - 6, 4) / 64._4
        enddo
     enddo
  enddo
  do k = 0, nz
     do j = 0, ny+1
        do i = 0, nx+1
           w4(i,j,k) = real(mod(3*i + 5*j + 7*k, 17) - 8, 4) / 64._4
           if (k >= 1) w4(i,j,k) = w4(i,j,k) - 1._4
        enddo
     enddo
  enddo
  allocate(u8(1:nx+1,0:ny+1,1:nz), v8(0:nx+1,1:ny+1,1:nz), w8(0:nx+1,0:ny+1,0:nz))
  u8 = real(u4, 8); v8 = real(v4, 8); w8 = real(w4, 8)

  call nhydro_solve(nx, ny, nz, rmask, u8, v8, w8)
  nite8 = iterations_in_history()
  call nhydro_solve_r4(nx, ny, nz, rmask, u4, v4, w4)
  nite4 = iterations_in_history()

  write(*,'(A,I0)') 'bits_differ_u = ', count(transfer(real(u8, 4), (/ 0_4 /)) /= transfer(u4, (/ 0_4 /)))
  write(*,'(A,I0)') 'bits_differ_v = ', count(transfer(real(v8, 4), (/ 0_4 /)) /= transfer(v4, (/ 0_4 /)))
  write(*,'(A,I0)') 'bits_differ_w = ', count(transfer(real(w8, 4), (/ 0_4 /)) /= transfer(w4, (/ 0_4 /)))
  write(*,'(A,I0)') 'nite_r8 = ', nite8
  write(*,'(A,I0)') 'nite_r4 = ', nite4
  call nhydro_check_nondivergence_r4(nx, ny, nz, rmask, u4, v4, w4)
  call nhydro_clean()

contains

  !> fort.100 holds one line for the starting residual and one per iteration of the solve that has just ended; read, then removed
  integer(kind=4) function iterations_in_history()
    integer :: ios
    character(len=8) :: line
    iterations_in_history = -1
    open(unit=22, file='fort.100', status='old', iostat=ios)
    if (ios /= 0) return
    do
       read(22,'(A)', iostat=ios) line
       if (ios /= 0) exit
       iterations_in_history = iterations_in_history + 1
    enddo
    close(22, status='delete')
  end function iterations_in_history

  subroutine forget_history()
    integer :: ios
    open(unit=22, file='fort.100', status='old', iostat=ios)
    if (ios == 0) close(22, status='delete')
  end subroutine forget_history
end program mg_testsolve_r4_gpu
