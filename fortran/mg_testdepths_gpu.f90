!> The matrices from the caller's own depths through the Fortran boundary (nhydro_matrices_depths, fortran/nhydro.f90): a flat bottom at
!> 32x32x16 under a free surface of 0.3 m and a stretched coordinate, four colours to 1e-8.  The program runs nhydro_matrices and
!> nhydro_solve, fetches zr and zw of level 1 through grid_get, cleans, initialises again, and runs nhydro_matrices_depths with them and
!> the same nhydro_solve.  On a flat bottom the coarsening rule of the depths is the sigma hierarchy bit for bit (DESIGN.md 6.4), so the
!> residuals the two solves print are equal character for character.  The line "---- depths ----" marks the second set-up in the program's
!> own output (the library prints through C's stdio: under a pipe its lines are buffered apart from the program's).
!> Parameters: ./nh_namelist when there is one (the tests write it), else the program writes the one named above.
program mg_testdepths_gpu
  use iso_c_binding
  use nhydro
  implicit none
  integer(kind=4), parameter :: nx = 32, ny = 32, nz = 16
  integer(kind=4) :: i, j, k, pass
  real(kind=8) :: hc, theta_b, theta_s
  real(kind=8), dimension(:,:), pointer :: dx, dy, zeta, h, rmask
  real(kind=8), dimension(:,:,:), allocatable :: zr, zw, u, v, w
  logical :: there

  inquire(file='nh_namelist', exist=there)
  if (.not. there) then
     open(unit=21, file='nh_namelist', status='new', action='write')
     write(21,'(A)') '&nhparam', " relax_method = 'FC',", ' solver_prec = 1.d-8,', '/'
     close(21)
  endif

  hc = 250._8; theta_b = 0.4_8; theta_s = 6._8
  allocate(dx(0:ny+1,0:nx+1), dy(0:ny+1,0:nx+1), zeta(0:ny+1,0:nx+1), h(0:ny+1,0:nx+1), rmask(0:ny+1,0:nx+1))
  do i = 0, nx+1
     do j = 0, ny+1
        dx(j,i) = 312.5_8 * (1._8 + 0.2_8 * sin(0.3_8 * real(i,kind=8)))     ! a metric that varies in i and in j
        dy(j,i) = 312.5_8 * (1._8 + 0.1_8 * cos(0.2_8 * real(j,kind=8)))
     enddo
  enddo
  zeta(:,:) = 0.3_8; h(:,:) = 3000._8; rmask(:,:) = 1._8
  allocate(zr(nz,-1:ny+2,-1:nx+2), zw(nz+1,-1:ny+2,-1:nx+2))
  allocate(u(1:nx+1,0:ny+1,1:nz), v(0:nx+1,1:ny+1,1:nz), w(0:nx+1,0:ny+1,0:nz))

  do pass = 1, 2
     call nhydro_init(nx, ny, nz, 1, 1)
     if (pass == 1) then
        call nhydro_matrices(dx, dy, zeta, h, rmask, hc, theta_b, theta_s)
        call grid_get(1, 'zr', zr)
        call grid_get(1, 'zw', zw)
     else
        write(*,'(A)') '---- depths ----'
        call nhydro_matrices_depths(dx, dy, zr, zw, rmask)
     endif
     do k = 1, nz
        do j = 0, ny+1
           do i = 1, nx+1
              u(i,j,k) = real(mod(7*i + 3*j + 5*k, 11) - 5, 8) / 64._8
           enddo
        enddo
        do j = 1, ny+1
           do i = 0, nx+1
              v(i,j,k) = real(mod(5*i + 7*j + 3*k, 13) - 6, 8) / 64._8
           enddo
        enddo
     enddo
     do k = 0, nz
        do j = 0, ny+1
           do i = 0, nx+1
              w(i,j,k) = real(mod(3*i + 5*j + 7*k, 17) - 8, 8) / 64._8
           enddo
        enddo
     enddo
     call nhydro_solve(nx, ny, nz, rmask, u, v, w)
     call nhydro_clean()
  enddo
end program mg_testdepths_gpu
